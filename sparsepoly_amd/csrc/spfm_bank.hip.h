// spfm_bank.hip.h -- a bank of F fitted models evaluated in one pass over the rows of X, and the
// per-row reductions fused behind it (argmax, loss sums, weighted mean).  Part of the gfx950
// device code; see DESIGN.md section 17.
//
// Layout.  The models share the kind (degree M or all-subsets), fit_lower, fit_linear and the
// column count d; they may differ in their component counts k_f.  Their parameters are stacked
// along the component axis, feature-major: per block Pt[d][S] with S = sum_f k_f, lams[S],
// w[d][F], and koff[F + 1] (model f owns the stacked components koff[f] .. koff[f+1] - 1).  One
// stored entry (i, j) then costs ONE contiguous read of S doubles for all models, and the row's
// indices and values are read once.
//
// Work split.  One wavefront per row.  The row's entries are staged in LDS, kBankStage at a time;
// the lanes run over the stacked components in chunks of 64, each lane the DP of
// anova_predict_kernel (a[t] += a[t-1] p x, entries in stored order) for its component.  A row of
// at most kBankStage entries is staged once for all chunks; a longer row is swept tile by tile
// for every chunk.  During the first chunk's sweep lane f < F also forms model f's linear term.
//
// Summation order (what the error bound of tests/test_hip_bank.py is derived from).  For model f
//   B_q  = ((0 + t_0) + t_1) + ... + t_{k_f - 1},  t_c = a_M(component c of f) * lams_c,
// the terms of block q added ONE AFTER THE OTHER IN THE MODEL'S OWN COMPONENT ORDER by lane f:
// after each chunk the 64 terms go through LDS and lane f adds those of them that are its own,
// in index order, to its running sum.  No butterfly, no atomics: where a chunk boundary falls
// inside a model changes nothing, a chunk that straddles two models feeds two lanes.
//   lin  = ((0 + x_1 w_1f) + x_2 w_2f) + ...   in stored order (as linear_predict_kernel)
//   score_f = (B_0 + lin) + B_1                (lin only with fit_linear, B_1 only with a second block)
// Every operand is model f's own, so the value depends neither on the other members nor on f's
// position, nor on the slab or the grid.
#pragma once
#include "spfm_common.hip.h"

namespace spfm {

constexpr int kBankStage = 128;            // entries of a row a wave stages at a time
constexpr int kBankMaxModels = 64;         // one model per lane of the wave that owns the row
constexpr int kBankMaxComponents = 4096;   // stacked components: 64 chunk sweeps per row at most

enum { BANK_SCORES = 0, BANK_ARGMAX = 1, BANK_LOSSES = 2, BANK_MEAN = 3 };

// One block of the bank on the rows of one slab: out[row][f] = B + lin (first) or += B.
// rptr holds the slab's rows with the matrix's own offsets, ridx / rval its entries from e0 on.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void bank_predict_kernel(
    int64_t rows, int64_t e0, int S, int F, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval,
    const double* __restrict__ Pt /* d x S */, const double* __restrict__ lams /* S */,
    const int32_t* __restrict__ koff /* F + 1 */, const double* __restrict__ wb /* d x F or NULL */,
    int first, double* __restrict__ out /* rows x F */) {
    __shared__ int32_t sh_j[kBlock / kWave][kBankStage];
    __shared__ double sh_x[kBlock / kWave][kBankStage];
    __shared__ double sh_t[kBlock / kWave][kWave];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (row >= rows) return;  // (waves are independent: no workgroup barrier below)
    const int64_t b = rptr[row] - e0;
    const int n_i = (int)(rptr[row + 1] - rptr[row]);
    const int ntile = (n_i + kBankStage - 1) / kBankStage;
    const int lo = lane < F ? koff[lane] : 0, hi = lane < F ? koff[lane + 1] : 0;
    int32_t* const js = sh_j[wave];
    double* const xs = sh_x[wave];
    double* const ts = sh_t[wave];
    double acc = 0.0, lin = 0.0;
    for (int c0 = 0; c0 < S; c0 += kWave) {
        const int s = c0 + lane;
        const bool active = s < S;
        const auto px = [&](int u) { return Pt[(size_t)js[u] * S + s] * xs[u]; };
        double a[M + 1];
        anova_dp_init<M>(a);
        for (int tile = 0; tile < ntile; ++tile) {
            const int len = min(kBankStage, n_i - tile * kBankStage);
            if (ntile > 1 || c0 == 0) {  // a short row stays staged for every chunk
                wave_lds_sync();         // the previous tile has been read
                for (int u = lane; u < len; u += kWave) {
                    const int64_t ii = b + (int64_t)tile * kBankStage + u;
                    js[u] = ridx[ii];
                    xs[u] = (double)rval[ii];
                }
                wave_lds_sync();
            }
            if (c0 == 0 && wb != nullptr && lane < F)
                for (int u = 0; u < len; ++u) lin += xs[u] * wb[(size_t)js[u] * F + lane];
            if (active) {
                if constexpr (M == 0)  // all-subsets kernel, as anova_predict_kernel
                    subsets_dp_add(a[0], 0, len, px);
                else
                    anova_dp_add<M>(a, 0, len, px);
            }
        }
        wave_lds_sync();  // the previous chunk's terms have been read
        ts[lane] = active ? a[M] * lams[s] : 0.0;
        wave_lds_sync();
        const int s0 = max(lo, c0), s1 = min(hi, c0 + kWave);
        for (int c = s0; c < s1; ++c) acc += ts[c - c0];
    }
    if (lane < F) {
        double* o = out + (size_t)row * F + lane;
        if (first)
            *o = (wb != nullptr) ? acc + lin : acc;
        else
            *o += acc;
    }
}

// per row: index of the largest score (ties: the lowest index), that score, the runner-up
static __global__ __launch_bounds__(kBlock) void bank_argmax_kernel(
    int64_t rows, int F, const double* __restrict__ sc, int32_t* __restrict__ idx,
    double* __restrict__ best, double* __restrict__ runner) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows) return;
    const double* r = sc + (size_t)i * F;
    double bv = r[0], rv = -INFINITY;
    int bi = 0;
    for (int f = 1; f < F; ++f) {
        const double v = r[f];
        if (v > bv) {
            rv = bv;
            bv = v;
            bi = f;
        } else if (v > rv) {
            rv = v;
        }
    }
    idx[i] = bi;
    best[i] = bv;
    runner[i] = rv;
}

// per row: ((0 + wt_0 s_0) + wt_1 s_1) + ... in model order
static __global__ __launch_bounds__(kBlock) void bank_mean_kernel(
    int64_t rows, int F, const double* __restrict__ sc, const double* __restrict__ wt,
    double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows) return;
    const double* r = sc + (size_t)i * F;
    double a = 0.0;
    for (int f = 0; f < F; ++f) a += wt[f] * r[f];
    out[i] = a;
}

// partial[block][f] = sum over the block's 256 rows of loss(score_if, y_if): one row per thread,
// block_sum2 (butterfly, then the four waves in order).  y[i * ys_row + f * ys_f]: shared target
// (1, 0) or per-model targets (F, 1).  Finished by bank_loss_finish_kernel.
static __global__ __launch_bounds__(kBlock) void bank_loss_partial_kernel(
    int64_t rows, int F, const double* __restrict__ sc, const double* __restrict__ y, int ys_row,
    int ys_f, int loss, double* __restrict__ partial) {
    __shared__ double red[16];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int f = 0; f < F; ++f) {
        double a = 0.0, b = 0.0;
        if (i < rows)
            a = loss_dev(loss, sc[(size_t)i * F + f], y[(size_t)i * ys_row + (size_t)f * ys_f]);
        block_sum2(a, b, red);
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * F + f] = a;
    }
}

// out[f] = sum of partial[0..P)[f]: workgroup f, thread t adds the partials t, t + 256, ... in
// order, then block_sum2 (fixed order => reproducible for one partition of the rows)
static __global__ __launch_bounds__(kBlock) void bank_loss_finish_kernel(
    int64_t P, int F, const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double red[16];
    const int f = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t p = threadIdx.x; p < P; p += kBlock) a += partial[(size_t)p * F + f];
    block_sum2(a, b, red);
    if (threadIdx.x == 0) out[f] = a;
}

// ------------------------------------------------------------------------------------------------
// Grouped, weighted per-member sums (spfm_bank_group_sums):
//   out[q][f][g] = sum over rows i with group[i] == g of weight[i] * metric_q(score_if, y_if).
constexpr int kBankMaxGroups = 32;
constexpr int kBankMaxMetrics = 4;
enum { METRIC_ABS_ERROR = 16, METRIC_SIGN_ERROR = 17 };  // beside the three LOSS_* ids

// the value of one metric on one (score, target); the three losses are loss_dev itself
__device__ __forceinline__ double bank_metric_dev(int metric, double p, double y) {
    if (metric == METRIC_ABS_ERROR) return fabs(p - y);
    if (metric == METRIC_SIGN_ERROR) return ((p > 0) != (y > 0)) ? 1.0 : 0.0;  // base.py's predict
    return loss_dev(metric, p, y);
}

// partial[block][q][g][f] for the block's 256 rows (the same blocks, and the same part0 indexing,
// as bank_loss_partial_kernel).  One workgroup per block of 256 rows, four waves.
//
// Work split.  Wave w of the block owns its rows 64 w .. 64 w + 63 -- a function of the row number
// alone, never of F.  Lane f < F is member f: the loads sc[i * F + f] of a row are coalesced, the
// row's group id and weight are wave-uniform.  The metrics are taken one after the other, so that
// the table in LDS is tab[wave][g][f], 4 G F doubles: 64 KB at the caps (G = 32, F = 64), 3.2 KB
// for five folds of twenty members.  Lane f alone reads and writes column f of its wave's table.
//
// Summation order (what the error bound of tests/test_hip_bank_groups.py is derived from).  For
// metric q, member f and group g, with t_i = weight[i] * metric_q(score_if, y_if) (this bracketing:
// a weight of 1.0 changes no bit of the term; weight NULL multiplies by 1.0 all the same):
//   W_w = ((0 + t_i1) + t_i2) + ...   the rows of wave w that belong to g, IN ROW ORDER: a row's
//                                     term goes through at most 64 additions;
//   B   = (((0 + W_0) + W_1) + W_2) + W_3   the four waves in wave order: 4 additions;
//   out = ((0 + B_0) + B_1) + ... + B_{P-1}  bank_group_finish_kernel, the P blocks of the call
//                                     IN BLOCK ORDER across all slabs: P additions.
// So a term goes through at most 64 + 4 + P additions, P = the call's blocks of 256 rows (every
// slab starts a new block).  No butterfly, no atomics, every operand is member f's own: the value
// depends neither on the other members nor on f's position nor on F, and for one slab size it is
// the same from run to run.  A group without rows sums nothing: exact zeros.
static __global__ __launch_bounds__(kBlock) void bank_group_partial_kernel(
    int64_t rows, int F, const double* __restrict__ sc, const double* __restrict__ y, int ys_row,
    int ys_f, const double* __restrict__ weight /* rows or NULL */,
    const int32_t* __restrict__ group /* rows or NULL */, int G, int Q, int4 metrics,
    double* __restrict__ partial /* blocks x Q x G x F */) {
    extern __shared__ double bank_group_tab[];  // [kBlock / kWave][G][F]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int GF = G * F;
    double* const tab = bank_group_tab + (size_t)wave * GF;
    const int64_t i0 = (int64_t)blockIdx.x * kBlock + (int64_t)wave * kWave;
    const int len = (int)max((int64_t)0, min((int64_t)kWave, rows - i0));
    for (int q = 0; q < Q; ++q) {
        const int metric = q == 0 ? metrics.x : q == 1 ? metrics.y : q == 2 ? metrics.z : metrics.w;
        if (lane < F) {
            for (int g = 0; g < G; ++g) tab[g * F + lane] = 0.0;
            for (int r = 0; r < len; ++r) {
                const int64_t i = i0 + r;
                const int g = group ? group[i] : 0;  // in [0, G): checked on the host
                const double w = weight ? weight[i] : 1.0;
                const double v = bank_metric_dev(metric, sc[(size_t)i * F + lane],
                                                 y[(size_t)i * ys_row + (size_t)lane * ys_f]);
                tab[g * F + lane] += w * v;
            }
        }
        __syncthreads();
        double* const o = partial + ((size_t)blockIdx.x * Q + q) * GF;
        for (int c = threadIdx.x; c < GF; c += kBlock) {
            double a = 0.0;
            for (int w = 0; w < kBlock / kWave; ++w) a += bank_group_tab[(size_t)w * GF + c];
            o[c] = a;
        }
        __syncthreads();  // the tables are zeroed again for the next metric
    }
}

// acc[q][g][f] += the slab's partials one after the other in block order: thread c owns cell c of
// the Q G F cells.  Run once per slab on the same accumulator (zeroed before the first slab), so
// the call's blocks are added in block order whatever the slabs are.
static __global__ __launch_bounds__(kBlock) void bank_group_finish_kernel(
    int64_t P, int cells, const double* __restrict__ partial, double* __restrict__ acc) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= cells) return;
    double a = acc[c];
#pragma unroll 8  // (the loads of eight blocks in flight; the additions stay in block order)
    for (int64_t p = 0; p < P; ++p) a += partial[(size_t)p * cells + c];
    acc[c] = a;
}

}  // namespace spfm
