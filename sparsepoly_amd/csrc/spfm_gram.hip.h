// spfm_gram.hip.h -- Gram matrices of sparsepoly.kernels (kernels.py:51-153) on the device
// Part of the gfx950 device code of the sparse-FM core; host side in spfm_engine_gram.hip,
// DESIGN.md section "Gram matrices".
//
// All three kernels of kernels.py are functions of the multiset {x_c * p_c : c in both supports}:
//   anova (kernels.py:71-115)        the DP a[t] += a[t-1] * v (pcd.py:23-30), value a[degree]
//   poly  (kernels.py:51-68)         (sum v) ** degree
//   all-subsets (kernels.py:117-137) prod (1 + v)
// One accumulator per kind (GramAcc) and two producers of the products:
//   gram_dense_kernel  CSR rows of X against a dense operand held transposed (d x ldp): lanes over
//                      output columns, the X row's entries staged in LDS once per workgroup
//   gram_csr_kernel    CSR rows of X against CSR rows of P: a merge of two sorted index lists,
//                      the P tile's entries staged in LDS when they fit
// Both write either the Gram block or, with lams, per-row partial sums of K * lams over one
// 64-column chunk (a fixed butterfly over the chunk's lanes; the host folds the chunks in
// column order).  No atomics: the result does not depend on how the host tiles the problem.
#pragma once
#include "spfm_common.hip.h"

namespace spfm {

enum { GRAM_ANOVA = 0, GRAM_POLY = 1, GRAM_ALL_SUBSETS = 2 };  // SPFM_GRAM_*

constexpr int kGramChunk = 64;        // output columns per lane group (one wave)
constexpr int kGramStage = 1024;      // X entries staged per round (dense path), 12 KiB of LDS
constexpr int kGramStageP = 2048;     // P-tile entries staged (CSR path), 24 KiB of LDS

// ANOVA DP state in registers: capacity CAP handles any runtime degree <= CAP.  The state is
// shifted so that the wanted order always lands in a[CAP]: a[CAP - degree] starts at 1 and the
// slots below it stay 0, so a[CAP - degree + t] runs exactly the DP of order t.  Every index is a
// compile-time constant (a runtime index would put the array in scratch).
template <int T>
__device__ __forceinline__ void anova_push(double* a, double v) {
    a[T] += a[T - 1] * v;
    if constexpr (T > 1) anova_push<T - 1>(a, v);
}

template <int KIND, int CAP>
struct GramAcc {
    double a[CAP + 1];
    __device__ __forceinline__ void init(int degree) {
#pragma unroll
        for (int t = 0; t <= CAP; ++t) a[t] = (t == CAP - degree) ? 1.0 : 0.0;
    }
    __device__ __forceinline__ void push(double v) { anova_push<CAP>(a, v); }
    __device__ __forceinline__ double value(int) const { return a[CAP]; }
};

template <int CAP>
struct GramAcc<GRAM_POLY, CAP> {
    double s;
    __device__ __forceinline__ void init(int) { s = 0.0; }
    __device__ __forceinline__ void push(double v) { s += v; }
    // polynomial_kernel(gamma=1, coef0=0): K **= degree
    __device__ __forceinline__ double value(int degree) const {
        if (degree == 0) return 1.0;
        if (degree == 1) return s;
        if (degree == 2) return s * s;
        return pow(s, (double)degree);
    }
};

template <int CAP>
struct GramAcc<GRAM_ALL_SUBSETS, CAP> {
    double p;
    __device__ __forceinline__ void init(int) { p = 1.0; }
    __device__ __forceinline__ void push(double v) { p *= 1 + v; }
    __device__ __forceinline__ double value(int) const { return p; }
};

struct GramDenseArgs {
    int rows;                   // X rows of this block
    int n2t;                    // output columns of this tile
    int group;                  // lane-group width: next power of two >= n2t, capped at 64
    int cpw;                    // 64-column chunks per workgroup row (1, 2 or 4)
    int degree;
    int lams_mode;              // 1: write chunk partial sums of K * lams instead of K
    int transpose_out;          // K block written (n2t x rows) instead of (rows x n2t)
    int n_chunks;               // 64-column chunks of this tile (row stride of `part`)
    int64_t ebase;              // rptr[0]: entries of this block start at ridx[0]
    const int64_t* rptr;        // rows + 1, absolute offsets
    const int32_t* ridx;
    const double* rval;
    const double* Bt;           // (d x ldp): column j of the tile at Bt[c * ldp + j]
    int64_t ldp;
    const double* lams;         // n2t (this tile's slice), lams_mode only
    double* out;                // K block, or part[rows][n_chunks]
};

// Workgroup = 256 lanes = 256/group lane groups.  Group q takes row q / cpw of the workgroup's
// row block and 64-column chunk blockIdx.y * cpw + q % cpw.  The block's X entries (one contiguous
// CSR range) are staged in LDS in rounds of kGramStage; every group keeps its accumulator in
// registers across the rounds, so a row of any length is read from HBM once per workgroup.
template <int KIND, int CAP>
__global__ __launch_bounds__(kBlock) void gram_dense_kernel(GramDenseArgs g) {
    __shared__ int32_t s_idx[kGramStage];
    __shared__ double s_val[kGramStage];
    const int tid = threadIdx.x;
    const int G = g.group;
    const int q = tid / G, lane = tid - q * G;
    const int rows_per_wg = (kBlock / G) / g.cpw;
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t rlast = min((int64_t)g.rows, row0 + rows_per_wg);  // exclusive
    const int64_t row = row0 + q / g.cpw;
    const int chunk = blockIdx.y * g.cpw + q % g.cpw;
    const int j = chunk * kGramChunk + lane;
    const bool row_ok = row < g.rows && chunk < g.n_chunks;
    const bool col_ok = row_ok && j < g.n2t;
    const int64_t wb = g.rptr[row0] - g.ebase, we = g.rptr[rlast] - g.ebase;
    int64_t b = 0, e = 0;
    if (row_ok) {
        b = g.rptr[row] - g.ebase;
        e = g.rptr[row + 1] - g.ebase;
    }
    const double* __restrict__ Bj = g.Bt + (col_ok ? j : 0);
    GramAcc<KIND, CAP> acc;
    acc.init(g.degree);
    for (int64_t s0 = wb; s0 < we; s0 += kGramStage) {
        const int ns = (int)min((int64_t)kGramStage, we - s0);
        __syncthreads();  // the previous round's readers are done
        for (int t = tid; t < ns; t += kBlock) {
            s_idx[t] = g.ridx[s0 + t];
            s_val[t] = g.rval[s0 + t];
        }
        __syncthreads();
        if (col_ok) {
            const int lo = (int)(max(b, s0) - s0), hi = (int)(min(e, s0 + ns) - s0);
            for (int t = lo; t < hi; ++t)
                acc.push(s_val[t] * Bj[(size_t)s_idx[t] * g.ldp]);
        }
    }
    double kv = col_ok ? acc.value(g.degree) : 0.0;
    if (g.lams_mode) {
        kv = col_ok ? kv * g.lams[j] : 0.0;
        kv = group_sum(kv, G);  // padding lanes add exact zeros: the same tree for any G
        if (row_ok && lane == 0) g.out[row * g.n_chunks + chunk] = kv;
    } else if (col_ok) {
        if (g.transpose_out)
            g.out[(size_t)j * g.rows + row] = kv;
        else
            g.out[(size_t)row * g.n2t + j] = kv;
    }
}

struct GramCsrArgs {
    int rows;                   // X rows of this block
    int n2t;                    // P rows of this tile
    int degree;
    int lams_mode;
    int stage_p;                // the tile's P entries fit kGramStageP: read them from LDS
    int n_chunks;               // 64-row chunks of this tile
    int64_t xbase;              // xptr[0]
    const int64_t* xptr;        // rows + 1
    const int32_t* xidx;
    const double* xval;
    int64_t pbase;              // pptr[0]
    const int64_t* pptr;        // n2t + 1
    const int32_t* pidx;
    const double* pval;
    const double* lams;         // n2t
    double* out;                // (rows x n2t) or part[rows][n_chunks]
};

// Workgroup = 4 waves; blockIdx.y = 64-row chunk of the P tile (lane = P row), each wave walks
// the rows of X r = blockIdx.x * 4 + wave, stepping by 4 * gridDim.x.  Output (r, j) is the merge
// of X row r and P row j, both sorted and duplicate-free; the products are pushed in feature
// order, as on the dense path (whose extra products are exact zeros).
template <int KIND, int CAP>
__global__ __launch_bounds__(kBlock) void gram_csr_kernel(GramCsrArgs g) {
    __shared__ int32_t s_idx[kGramStageP];
    __shared__ double s_val[kGramStageP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = blockIdx.y * kGramChunk + lane;
    const bool col_ok = j < g.n2t;
    const int jlo = blockIdx.y * kGramChunk;
    const int jhi = min(g.n2t, jlo + kGramChunk);
    // entries of this chunk's P rows: staged once per workgroup when they fit
    const int64_t cb = g.pptr[jlo] - g.pbase, ce = g.pptr[jhi] - g.pbase;
    const int32_t* pidx = g.pidx;
    const double* pval = g.pval;
    int64_t pofs = 0;
    if (g.stage_p) {
        for (int64_t t = tid; t < ce - cb; t += kBlock) {
            s_idx[t] = g.pidx[cb + t];
            s_val[t] = g.pval[cb + t];
        }
        __syncthreads();
        pidx = s_idx;
        pval = s_val;
        pofs = cb;
    }
    int64_t pb = 0, pe = 0;
    if (col_ok) {
        pb = g.pptr[j] - g.pbase - pofs;
        pe = g.pptr[j + 1] - g.pbase - pofs;
    }
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < g.rows; r += (int64_t)gridDim.x * 4) {
        const int64_t xb = g.xptr[r] - g.xbase, xe = g.xptr[r + 1] - g.xbase;
        GramAcc<KIND, CAP> acc;
        acc.init(g.degree);
        if (col_ok) {
            int64_t u = xb, w = pb;
            while (u < xe && w < pe) {
                const int32_t cu = g.xidx[u], cw = pidx[w];
                if (cu == cw) {
                    acc.push(g.xval[u] * pval[w]);
                    ++u;
                    ++w;
                } else if (cu < cw) {
                    ++u;
                } else {
                    ++w;
                }
            }
        }
        double kv = col_ok ? acc.value(g.degree) : 0.0;
        if (g.lams_mode) {
            kv = col_ok ? kv * g.lams[j] : 0.0;
            kv = wave_sum(kv);
            if (lane == 0) g.out[r * g.n_chunks + blockIdx.y] = kv;
        } else if (col_ok) {
            g.out[(size_t)r * g.n2t + j] = kv;
        }
    }
}

}  // namespace spfm
