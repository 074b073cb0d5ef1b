// spfm_explain.hip.h -- per-row feature attributions (exact Shapley values against a zero
// baseline), input gradients on the stored entries, row sums and the per-row top-K.
// Part of the gfx950 device code of the sparse-FM core; see DESIGN.md section 16.
//
// A block of the model is sum_s lams_s sum_t c[s][t] A^t(p_s, x).  Every monomial of A^t splits
// equally among its t members, and A^t restricted to the monomials that hold entry j is
// p_sj x_ij A^{t-1}(p_s, x_i without j), so
//   phi_ij  = w_j x_ij + x_ij sum_s lams_s p_sj sum_t (c[s][t] / t) g_{t-1}
//   df/dx_ij = w_j     +      sum_s lams_s p_sj sum_t  c[s][t]      g_{t-1}
// with g_0 = 1, g_t = a_t - p_sj x_ij g_{t-1} (a_t the kernel of the whole row: the downdate of
// grad_factor<M>, spfm_common.hip.h).
#pragma once
#include "spfm_common.hip.h"

namespace spfm {

constexpr int kExplainMaxK = 64;  // SPFM_EXPLAIN_MAX_K
constexpr int kExplainChunk = 64;  // components per LDS table: one per lane of phase A
constexpr int kExplainCoefs = 7;   // c[s][0..6], column 0 unused on the device
enum { EXPLAIN_ATTRIBUTION = 0, EXPLAIN_GRADIENT = 1 };

// out[e] = w_j x_e (attribution), w_j (gradient) or 0 (no linear term): the first term of every
// entry, the blocks add to it in launch order
template <typename T>
__global__ __launch_bounds__(kBlock) void explain_init_kernel(
    int64_t ne, const int32_t* __restrict__ ridx, const T* __restrict__ rval,
    const double* __restrict__ w /* or NULL */, int mode, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= ne) return;
    double v = 0.0;
    if (w != nullptr) {
        v = w[ridx[e]];
        if (mode == EXPLAIN_ATTRIBUTION) v *= (double)rval[e];
    }
    out[e] = v;
}

// One block of degree M added into out: one wave per row, components in chunks of 64.
//   phase A  lanes over the chunk's components, as anova_predict_kernel: a_1 .. a_{M-1} of the
//            whole row and lams_s c[s][t] (/ t) into the wave's LDS table, [value][component]
//   phase B  lanes over the row's entries: each walks the chunk's components in index order,
//            reads the table (one address per wave instruction: a broadcast) and its own row of
//            Pt (d,k), runs the downdate and adds one value to its entry
// No atomics, no cross-lane sum; an entry is always handled by one lane, chunks in order, so its
// bits depend on the row alone.  rptr holds the matrix's own offsets, e0 the slab's first entry.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void explain_block_kernel(
    int64_t rows, int k, int64_t e0, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const double* __restrict__ Pt,
    const double* __restrict__ lams, const double* __restrict__ coef /* k x 7 */, int mode,
    double* __restrict__ out) {
    __shared__ double tab[kBlock / kWave][2 * M - 1][kExplainChunk];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (row >= rows) return;  // (waves are independent: no workgroup barrier below)
    const int64_t b = rptr[row] - e0, e = rptr[row + 1] - e0;
    if (b == e) return;
    double(*tw)[kExplainChunk] = tab[wave];
    for (int s0 = 0; s0 < k; s0 += kExplainChunk) {
        const int s = s0 + lane;
        if (s < k) {
            double a[M];
            anova_dp_init<M - 1>(a);
            anova_dp_add<M - 1>(a, b, e, [&](int64_t ii) {
                return Pt[(size_t)ridx[ii] * k + s] * (double)rval[ii];
            });
#pragma unroll
            for (int t = 1; t < M; ++t) tw[t - 1][lane] = a[t];
            const double lam = lams[s];
#pragma unroll
            for (int t = 1; t <= M; ++t) {
                double c = coef[(size_t)s * kExplainCoefs + t];
                if (mode == EXPLAIN_ATTRIBUTION) c = c / (double)t;
                tw[M - 2 + t][lane] = lam * c;
            }
        }
        wave_lds_sync();
        const int ns = (k - s0 < kExplainChunk) ? k - s0 : kExplainChunk;
        for (int64_t ii = b + lane; ii < e; ii += kWave) {
            const double x = (double)rval[ii];
            const double* __restrict__ prow = Pt + (size_t)ridx[ii] * k + s0;
            double acc = 0.0;
            for (int sl = 0; sl < ns; ++sl) {
                const double p = prow[sl], px = p * x;
                double g = 1.0, inner = tw[M - 1][sl];
#pragma unroll
                for (int t = 2; t <= M; ++t) {
                    g = tw[t - 2][sl] - px * g;
                    inner += tw[M - 2 + t][sl] * g;
                }
                acc += p * inner;
            }
            if (mode == EXPLAIN_ATTRIBUTION) acc *= x;
            out[ii] += acc;
        }
        wave_lds_sync();  // the next chunk overwrites the table
    }
}

// rowsum[i] = sum_j out[i, j]: lane l adds the entries l, l + 64, ... in order, then the fixed
// butterfly of wave_sum
static __global__ __launch_bounds__(kBlock) void explain_rowsum_kernel(
    int64_t rows, int64_t e0, const int64_t* __restrict__ rptr, const double* __restrict__ vals,
    double* __restrict__ rowsum) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int64_t b = rptr[row] - e0, e = rptr[row + 1] - e0;
    double acc = 0.0;
    for (int64_t ii = b + lane; ii < e; ii += kWave) acc += vals[ii];
    acc = wave_sum(acc);
    if (lane == 0) rowsum[row] = acc;
}

// (|value| descending, column ascending, position ascending): a strict total order on a row's
// entries.  mag = the bits of |value| (monotone for non-negative doubles; a NaN sorts first).
// The comparison is one boolean expression and explain_take selects all four fields under one
// mask, so a selection round is straight-line code.
struct ExplainKey {
    long long mag;  // -1: no entry (loses to every entry)
    int col, pos;
    double val;
};
__device__ __forceinline__ bool explain_beats(const ExplainKey& a, const ExplainKey& b) {
    return (a.mag > b.mag) |
           ((a.mag == b.mag) & ((a.col < b.col) | ((a.col == b.col) & (a.pos < b.pos))));
}
__device__ __forceinline__ void explain_take(ExplainKey& best, const ExplainKey& c, bool take) {
    best.mag = take ? c.mag : best.mag;
    best.col = take ? c.col : best.col;
    best.pos = take ? c.pos : best.pos;
    best.val = take ? c.val : best.val;
}

// The per-row exact top-K of this unit and of the pair attributions: one wave selects the
// min(K, n) of a row's n values largest by |value|, in that order.  One exact selection round per
// slot: every lane finds the best of its values (l, l + 64, ...) that come strictly after the
// previous winner, a butterfly over the lanes picks the round's winner.  Integer comparisons only.
// col_of(p) is the key column of position p; COL = false: it is 0 for all (the order is by
// position alone) and is not carried through the butterfly.  Lane 0 calls write(q, best) for
// every slot; a slot past the row's values gets mag = pos = -1, val = 0 and column -1 (COL) or 0.
// (Not the streaming selection of spfm_select.hip.h: that one keeps sorted lists per strip and
// breaks ties by candidate id -- another algorithm with other tie rules.)
template <bool COL, typename ColFn, typename WriteFn>
__device__ __forceinline__ void explain_select(const double* __restrict__ vals, int n, int K,
                                               int lane, ColFn&& col_of, WriteFn&& write) {
    ExplainKey prev = {INT64_MAX, -1, -1, 0.0};  // every value comes after it
    for (int q = 0; q < K; ++q) {
        ExplainKey best = {-1, COL ? -1 : 0, -1, 0.0};
        if (q < n) {
            for (int p = lane; p < n; p += kWave) {
                const double v = vals[p];
                const ExplainKey c = {__double_as_longlong(fabs(v)), col_of(p), p, v};
                const bool after = explain_beats(prev, c), wins = explain_beats(c, best);
                explain_take(best, c, after && wins);
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                ExplainKey o;
                o.mag = __shfl_xor(best.mag, m, kWave);
                o.col = COL ? __shfl_xor(best.col, m, kWave) : best.col;
                o.pos = __shfl_xor(best.pos, m, kWave);
                o.val = __shfl_xor(best.val, m, kWave);
                explain_take(best, o, explain_beats(o, best));
            }
            prev = best;  // (q < n: there was a value left, in every lane's view the same)
        }
        if (lane == 0) write(q, best);
    }
}

// The min(K, n_i) entries of every row largest by |value|, in that order; the rest of the K slots
// hold column -1 and value 0.  One wave per row; the order is (|value|, column, position).
static __global__ __launch_bounds__(kBlock) void explain_topk_kernel(
    int64_t rows, int64_t e0, const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const double* __restrict__ vals, int K, int32_t* __restrict__ oidx,
    double* __restrict__ oval) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (row >= rows) return;
    const int64_t b = rptr[row] - e0;
    const int n = (int)(rptr[row + 1] - e0 - b);  // (the host refuses longer rows)
    int32_t* oi = oidx + (size_t)row * K;
    double* ov = oval + (size_t)row * K;
    explain_select<true>(
        vals + b, n, K, threadIdx.x & 63, [&](int p) { return ridx[b + p]; },
        [&](int q, const ExplainKey& best) {
            oi[q] = best.col;
            ov[q] = best.val;
        });
}

}  // namespace spfm
