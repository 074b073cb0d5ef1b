// spfm_pairs.hip.h -- per-row pair attributions (the Shapley-Taylor interaction index of order 2
// against a zero baseline), the mixed second derivative on the stored pairs, the per-row top-K
// of the pairs and the per-row group x group tables.
// Part of the gfx950 device code of the sparse-FM core; see DESIGN.md section 16a.
//
// A block of the model is sum_s lams_s sum_t c[s][t] A^t(p_s, x).  A monomial of one entry stays
// with that entry, a monomial of t >= 2 entries splits equally among its t (t - 1) / 2 pairs, and
// A^t restricted to the monomials that hold the entries a and b is z_sa z_sb A^{t-2}(p_s, x_i
// without a and b), z_sj = p_sj x_ij, so for the stored entries a < b of row i
//   main_ia        = w_a x_ia + sum_s lams_s c[s][1] z_sa
//   phi_iab        = sum_s lams_s z_sa z_sb sum_{t=2..M} c[s][t] 2 / (t (t - 1)) h_{t-2}
//   d2f/dx_a dx_b  = sum_s lams_s p_sa p_sb sum_{t=2..M} c[s][t]                 h_{t-2}
// with g_0 = h_0 = 1, g_t = a_t - z_sa g_{t-1}, h_t = g_t - z_sb h_{t-1} (a_t the kernel of the
// whole row): the downdate of spfm_explain.hip.h applied twice.
//
// The pairs of a row of n entries are numbered by (first position, second position):
// (a, b), a < b, is pair a n - a (a + 1) / 2 + b - a - 1 of its n (n - 1) / 2.
#pragma once
#include "spfm_explain.hip.h"

namespace spfm {

constexpr int kPairsMaxK = 64;        // SPFM_PAIRS_MAX_K
constexpr int kPairsMaxGroups = 32;   // SPFM_PAIRS_MAX_GROUPS
constexpr int kPairsMaxRow = 65536;   // entries of a row: its last pair index fits an int
enum { PAIRS_INTERACTION = 0, PAIRS_HESSIAN = 1 };

// the index of the first pair whose first member is position a (n <= 65536: below 2^31)
__device__ __forceinline__ long long pairs_row_start(int n, int a) {
    return (long long)a * (2ll * n - a - 1) / 2;
}

// pair index q in [0, n (n - 1) / 2) -> (a, b).  The root of a^2 - (2 n - 1) a + 2 q = 0 in
// double ((2 n - 1)^2 < 2^35 is exact), then put right with the integer starts.
__device__ __forceinline__ void pairs_decode(int n, int q, int& a, int& b) {
    const double m = 2.0 * n - 1.0;
    int c = (int)((m - sqrt(m * m - 8.0 * (double)q)) * 0.5);
    c = c < 0 ? 0 : (c > n - 2 ? n - 2 : c);
    while (c > 0 && pairs_row_start(n, c) > q) --c;
    while (c < n - 2 && pairs_row_start(n, c + 1) <= q) ++c;
    a = c;
    b = c + 1 + (int)(q - pairs_row_start(n, c));
}

// main[e] += sum_s lams_s c[s][1] p_sj x_e of one block: the monomials of one entry that a
// coefficient table (fit_lower='augment') puts beside the linear term, which explain_init_kernel
// has written.  One thread per entry, the components in index order.
template <typename T>
__global__ __launch_bounds__(kBlock) void pairs_main_kernel(
    int64_t ne, int k, const int32_t* __restrict__ ridx, const T* __restrict__ rval,
    const double* __restrict__ Pt, const double* __restrict__ lams,
    const double* __restrict__ coef /* k x 7 */, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= ne) return;
    const double x = (double)rval[e];
    const double* __restrict__ prow = Pt + (size_t)ridx[e] * k;
    double acc = 0.0;
    for (int s = 0; s < k; ++s)
        acc += (lams[s] * coef[(size_t)s * kExplainCoefs + 1]) * (prow[s] * x);
    out[e] += acc;
}

// One block of degree M added into the slab's pair values: one wave per row, components in
// chunks of 64.
//   phase A  lanes over the chunk's components, as explain_block_kernel: a_1 .. a_{M-2} of the
//            whole row and lams_s c[s][t] (/ (t (t - 1) / 2)), t = 2..M, into the wave's LDS
//            table, [value][component].  M = 2 needs no a_t: the row is not read here.
//   phase B  sweeps of 64 pairs, one per lane: the lane walks the chunk's components in index
//            order, reads the table (one address per wave instruction: a broadcast) and its two
//            rows of Pt (d,k), runs both downdates and adds one value to its pair
// No atomics, no cross-lane sum; a pair is always handled by one lane, chunks in order, so its
// bits depend on the row alone.  rptr holds the matrix's own offsets, e0 the slab's first entry;
// pptr the slab's pair offsets (rows + 1, from 0).
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void pairs_block_kernel(
    int64_t rows, int k, int64_t e0, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval,
    const int64_t* __restrict__ pptr, const double* __restrict__ Pt,
    const double* __restrict__ lams, const double* __restrict__ coef /* k x 7 */, int mode,
    double* __restrict__ pv) {
    constexpr int NA = M - 2;  // a_1 .. a_{M-2}, then the M - 1 coefficients
    __shared__ double tab[kBlock / kWave][2 * M - 3][kExplainChunk];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (row >= rows) return;  // (waves are independent: no workgroup barrier below)
    const int64_t b = rptr[row] - e0, e = rptr[row + 1] - e0;
    if (e - b < 2) return;
    const int n = (int)(e - b);  // (the host refuses rows of more than 65 536 entries)
    const int np = (int)(pptr[row + 1] - pptr[row]);
    double* __restrict__ out = pv + pptr[row];
    double(*tw)[kExplainChunk] = tab[wave];
    for (int s0 = 0; s0 < k; s0 += kExplainChunk) {
        const int s = s0 + lane;
        if (s < k) {
            if constexpr (M > 2) {
                double a[M - 1];
                anova_dp_init<M - 2>(a);
                anova_dp_add<M - 2>(a, b, e, [&](int64_t ii) {
                    return Pt[(size_t)ridx[ii] * k + s] * (double)rval[ii];
                });
#pragma unroll
                for (int t = 1; t < M - 1; ++t) tw[t - 1][lane] = a[t];
            }
            const double lam = lams[s];
#pragma unroll
            for (int t = 2; t <= M; ++t) {
                double c = coef[(size_t)s * kExplainCoefs + t];
                if (mode == PAIRS_INTERACTION) c = c / (double)(t * (t - 1) / 2);
                tw[NA + t - 2][lane] = lam * c;
            }
        }
        wave_lds_sync();
        const int ns = (k - s0 < kExplainChunk) ? k - s0 : kExplainChunk;
        for (int q0 = 0; q0 < np; q0 += kWave) {  // (np < 2^31 - 64: no overflow)
            const int q = q0 + lane;
            if (q < np) {
                int ia, ib;
                pairs_decode(n, q, ia, ib);
                const double xa = (double)rval[b + ia], xb = (double)rval[b + ib];
                const double* __restrict__ pra = Pt + (size_t)ridx[b + ia] * k + s0;
                const double* __restrict__ prb = Pt + (size_t)ridx[b + ib] * k + s0;
                double acc = 0.0;
                for (int sl = 0; sl < ns; ++sl) {
                    const double pa = pra[sl], pb = prb[sl];
                    double inner = tw[NA][sl];  // t = 2: h_0 = 1
                    if constexpr (M > 2) {
                        const double za = pa * xa, zb = pb * xb;
                        double g = 1.0, h = 1.0;
#pragma unroll
                        for (int t = 3; t <= M; ++t) {
                            g = tw[t - 3][sl] - za * g;
                            h = g - zb * h;
                            inner += tw[NA + t - 2][sl] * h;
                        }
                    }
                    acc += (pa * pb) * inner;
                }
                if (mode == PAIRS_INTERACTION) acc *= xa * xb;
                out[q] += acc;
            }
        }
        wave_lds_sync();  // the next chunk overwrites the table
    }
}

// The min(K, pairs of the row) pairs of every row largest by |value|, in that order; the rest of
// the K slots hold columns -1, -1 and value 0.  explain_select (spfm_explain.hip.h) over the row's
// pair values with the order (|value| descending, pair index ascending): the key's column is the
// same for all, its position is the pair index.  The winner's index is turned into the two
// columns when it is written.
static __global__ __launch_bounds__(kBlock) void pairs_topk_kernel(
    int64_t rows, int64_t e0, const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const int64_t* __restrict__ pptr, const double* __restrict__ pv, int K,
    int32_t* __restrict__ ocola, int32_t* __restrict__ ocolb, double* __restrict__ oval) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (row >= rows) return;
    const int64_t b = rptr[row] - e0;
    const int n = (int)(rptr[row + 1] - e0 - b);
    const int np = (int)(pptr[row + 1] - pptr[row]);
    int32_t* oa = ocola + (size_t)row * K;
    int32_t* ob = ocolb + (size_t)row * K;
    double* ov = oval + (size_t)row * K;
    explain_select<false>(
        pv + pptr[row], np, K, threadIdx.x & 63, [](int) { return 0; },
        [&](int r, const ExplainKey& best) {
            int ca = -1, cb = -1;
            if (r < np) {
                int ia, ib;
                pairs_decode(n, best.pos, ia, ib);
                ca = ridx[b + ia];
                cb = ridx[b + ib];
            }
            oa[r] = ca;
            ob[r] = cb;
            ov[r] = best.val;
        });
}

// Per row the upper-triangular G x G table of its pair values by the groups of the two members,
// cell (g, h), g <= h, at g G - g (g - 1) / 2 + h - g of G (G + 1) / 2, and main summed per
// group.  One wave per row; a lane owns a cell (64 cells per pass) and walks the row's pairs in
// ascending pair index, adding the ones that fall into its cell: no atomics, no cross-lane sum.
// The group ids of the two members are the same in all lanes (uniform loads).
static __global__ __launch_bounds__(kBlock) void pairs_group_kernel(
    int64_t rows, int64_t e0, const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const int64_t* __restrict__ pptr, const double* __restrict__ pv,
    const double* __restrict__ main, int G, const int32_t* __restrict__ grp /* d */,
    double* __restrict__ opairs /* rows x G (G + 1) / 2 */, double* __restrict__ omain) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int64_t b = rptr[row] - e0;
    const int n = (int)(rptr[row + 1] - e0 - b);
    const double* __restrict__ vals = pv + pptr[row];
    const int cells = G * (G + 1) / 2;
    for (int c0 = 0; c0 < cells; c0 += kWave) {
        const int cell = c0 + lane;
        double acc = 0.0;
        int q = 0;
        for (int ia = 0; ia + 1 < n; ++ia) {
            const int ga = grp[ridx[b + ia]];
            for (int ib = ia + 1; ib < n; ++ib, ++q) {
                const int gb = grp[ridx[b + ib]];
                const int lo = ga < gb ? ga : gb, hi = ga < gb ? gb : ga;
                if (lo * G - lo * (lo - 1) / 2 + hi - lo == cell) acc += vals[q];
            }
        }
        if (cell < cells) opairs[(size_t)row * cells + cell] = acc;
    }
    if (lane < G) {  // (G <= 32)
        double acc = 0.0;
        for (int ia = 0; ia < n; ++ia)
            if (grp[ridx[b + ia]] == lane) acc += main[b + ia];
        omain[(size_t)row * G + lane] = acc;
    }
}

}  // namespace spfm
