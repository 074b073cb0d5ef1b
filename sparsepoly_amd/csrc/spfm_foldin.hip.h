// spfm_foldin.hip.h -- fold-in of single columns: the design of the per-column convex problem
// and its damped Newton solve.  Part of the gfx950 device code of the sparse-FM core; see
// DESIGN.md section 18.
//
// The ANOVA kernel is multilinear: with every other column fixed, the output on a row i that
// stores the target column j is affine in that column's parameters,
//   f(x_i) = c_i + z_i . theta_j,   theta_j = (w_j ; p^{o_q}_{sj}),
//   z_i    = x_ij (1 ; lams_s sum_{t=1..M_q} c_q[s][t] A^{t-1}(p_s, x_i without j)),
//   c_i    = f(x_i without j).
// foldin_design_kernel forms (z_i, c_i) by a pass over the row that SKIPS the target entry (no
// downdate: no cancellation, and no bit depends on what column j holds); foldin_solve_kernel
// minimises F_j(theta) = sum_i loss(c_i + z_i . theta, y_i) + 1/2 theta' Lambda theta per column.
#pragma once
#include "spfm_common.hip.h"

namespace spfm {

constexpr int kFoldinMaxUnknowns = 128;  // SPFM_FOLDIN_MAX_UNKNOWNS
constexpr int kFoldinCoefs = 7;          // c[s][0..6]
constexpr int kFoldinChunk = 16;         // rows of Z staged in LDS at a time
constexpr int kFoldinHalvings = 40;      // of the line search
constexpr double kFoldinArmijo = 1e-4;

// Design row and offset of every participating row for block q of degree M: one wave per row,
// lanes over the components in chunks of 64.  rptr / ridx / rval: the group's rows (offsets from
// 0), tpos[row]: the position of the target entry within the row.  Z (rows x Rp): column
// zoff + s is written; the first block also writes the linear column, the padding and starts
// c (offset + linear term), later blocks add to it.
template <typename T, int M>
__global__ __launch_bounds__(kBlock) void foldin_design_kernel(
    int64_t rows, int k, int R, int Rp, int zoff, int first, int lin, double offset,
    const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const T* __restrict__ rval, const int32_t* __restrict__ tpos, const double* __restrict__ Pt,
    const double* __restrict__ w, const double* __restrict__ lams,
    const double* __restrict__ coef /* k x 7 */, double* __restrict__ Z, double* __restrict__ c) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (row >= rows) return;  // (waves are independent: no workgroup barrier below)
    const int64_t b = rptr[row], e = rptr[row + 1], tt = b + tpos[row];
    const double xt = (double)rval[tt];
    double* __restrict__ zrow = Z + (size_t)row * Rp;
    double cacc;
    if (first) {
        double l = 0.0;
        if (lin) {
            for (int64_t ii = b + lane; ii < e; ii += kWave)
                if (ii != tt) l += w[ridx[ii]] * (double)rval[ii];
            l = wave_sum(l);
            if (lane == 0) zrow[0] = xt;
        }
        cacc = offset + l;
        for (int a = R + lane; a < Rp; a += kWave) zrow[a] = 0.0;
    } else {
        cacc = c[row];
    }
    for (int s0 = 0; s0 < k; s0 += kWave) {
        const int s = s0 + lane;
        double v = 0.0;
        if (s < k) {
            const auto px = [&](int64_t ii) {
                return Pt[(size_t)ridx[ii] * k + s] * (double)rval[ii];
            };
            double a[M + 1];
            anova_dp_init<M>(a);
            // the row without its target entry: [b, tt), then [tt + 1, e) -- one copy of the loop
#pragma nounroll
            for (int half = 0; half < 2; ++half)
                anova_dp_add<M>(a, half ? tt + 1 : b, half ? e : tt, px);
            const double* __restrict__ cs = coef + (size_t)s * kFoldinCoefs;
            const double lam = lams[s];
            double zs = 0.0, cv = cs[0];
#pragma unroll
            for (int t = 1; t <= M; ++t) {
                zs += cs[t] * a[t - 1];
                cv += cs[t] * a[t];
            }
            zrow[zoff + s] = xt * (lam * zs);
            v = lam * cv;
        }
        cacc += wave_sum(v);
    }
    if (lane == 0) c[row] = cacc;
}

// l''(p): the derivative of the active branch of dloss_dev
__device__ __forceinline__ double d2loss_dev(int loss, double p, double y) {
    if (loss == LOSS_SQUARED) return 1.0;
    if (loss == LOSS_LOGISTIC) {
        const double z = p * y;
        if (z > 18.0) return (y * y) * exp(-z);
        if (z < -18.0) return 0.0;
        const double ez = exp(z), q = ez + 1.0;
        return (y * y) * ez / (q * q);
    }
    return (1 - p * y > 0) ? 2 * (y * y) : 0.0;
}

// entry e of a packed lower triangle -> (a, b), a >= b, e = a (a + 1) / 2 + b
__device__ __forceinline__ void foldin_tri(int e, int& a, int& b) {
    a = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    while (a * (a + 1) / 2 > e) --a;
    b = e - a * (a + 1) / 2;
}

// LDS of foldin_solve_kernel in doubles: H (packed triangle), a chunk of Z, theta / trial / g /
// step, per chunk row: margin-derived d1, d2, loss
__host__ __device__ inline size_t foldin_solve_lds(int R, int Rp) {
    return (size_t)R * (R + 1) / 2 + (size_t)kFoldinChunk * Rp + 4 * (size_t)Rp +
           3 * (size_t)kFoldinChunk + 8;
}

struct FoldinSolveArgs {
    int R, Rp, lin, loss, max_iter;
    double alpha, beta, tol;
    const int64_t* cptr;  // (columns + 1) first row of every column of the group
    const double* Z;      // rows x Rp
    const double* c;      // rows
    const double* y;      // rows
    double* theta;        // columns x R
    double* stat;         // columns x 3: max|grad|, F(0), F(theta)
    int32_t* it;          // columns x 2: iterations, converged
};

// One workgroup per target column.  Every sum over the column's rows is formed by ONE thread per
// entry that walks the rows in ascending order (the chunks only stage Z in LDS), so no bit
// depends on anything but the column's own rows.
//   pass(th, full): F(th) always; with `full` also g = Z' l' + Lambda th (sh_g) and
//                   H = Z' diag(l'') Z + Lambda (sh_H, packed lower triangle)
static __global__ __launch_bounds__(kBlock) void foldin_solve_kernel(FoldinSolveArgs A) {
    extern __shared__ __attribute__((aligned(16))) double fi_lds[];
    const int R = A.R, Rp = A.Rp, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ntri = R * (R + 1) / 2;
    double* sh_H = fi_lds;
    double* sh_z = sh_H + ntri;                   // [kFoldinChunk][Rp]
    double* sh_th = sh_z + kFoldinChunk * Rp;     // theta
    double* sh_tr = sh_th + Rp;                   // trial point
    double* sh_g = sh_tr + Rp;                    // gradient
    double* sh_s = sh_g + Rp;                     // Newton step
    double* sh_d1 = sh_s + Rp;                    // [kFoldinChunk]
    double* sh_d2 = sh_d1 + kFoldinChunk;
    double* sh_ls = sh_d2 + kFoldinChunk;
    double* sh_sc = sh_ls + kFoldinChunk;         // [8] scalars: 0 F, 1 flag, 2 value
    const int64_t col = blockIdx.x;
    const int64_t r0 = A.cptr[col], r1 = A.cptr[col + 1];

    auto lam_of = [&](int a) { return (A.lin && a == 0) ? A.alpha : A.beta; };

    auto pass = [&](const double* th, bool full) -> double {
        double gacc = 0.0;
        if (full)
            for (int e = tid; e < ntri; e += kBlock) sh_H[e] = 0.0;
        if (tid == 0) sh_sc[0] = 0.0;
        __syncthreads();
        for (int64_t rb = r0; rb < r1; rb += kFoldinChunk) {
            const int nr = (int)((r1 - rb < kFoldinChunk) ? r1 - rb : kFoldinChunk);
            const double* __restrict__ zsrc = A.Z + (size_t)rb * Rp;
            for (int e = tid; e < nr * Rp; e += kBlock) sh_z[e] = zsrc[e];
            __syncthreads();
            for (int r = wave; r < nr; r += kBlock / kWave) {
                double dot = 0.0;
                for (int a = lane; a < R; a += kWave) dot += sh_z[r * Rp + a] * th[a];
                dot = wave_sum(dot);
                if (lane == 0) {
                    const double p = A.c[rb + r] + dot, yv = A.y[rb + r];
                    sh_ls[r] = loss_dev(A.loss, p, yv);
                    sh_d1[r] = dloss_dev(A.loss, p, yv);
                    sh_d2[r] = d2loss_dev(A.loss, p, yv);
                }
            }
            __syncthreads();
            if (tid == 0) {
                double f = sh_sc[0];
                for (int r = 0; r < nr; ++r) f += sh_ls[r];
                sh_sc[0] = f;
            }
            if (full) {
                if (tid < R)
                    for (int r = 0; r < nr; ++r) gacc += sh_d1[r] * sh_z[r * Rp + tid];
                for (int e = tid; e < ntri; e += kBlock) {
                    int a, b;
                    foldin_tri(e, a, b);
                    double h = sh_H[e];
                    for (int r = 0; r < nr; ++r)
                        h += (sh_d2[r] * sh_z[r * Rp + a]) * sh_z[r * Rp + b];
                    sh_H[e] = h;
                }
            }
            __syncthreads();
        }
        if (full && tid < R) {
            sh_g[tid] = gacc + lam_of(tid) * th[tid];
            sh_H[tid * (tid + 1) / 2 + tid] += lam_of(tid);
        }
        if (tid == 0) {
            double reg = 0.0;
            for (int a = 0; a < R; ++a) reg += (0.5 * lam_of(a)) * (th[a] * th[a]);
            sh_sc[0] = sh_sc[0] + reg;
        }
        __syncthreads();
        const double F = sh_sc[0];
        __syncthreads();
        return F;
    };
    auto gmax = [&]() -> double {  // max|g|, the same in every thread
        if (tid == 0) {
            double m = 0.0;
            for (int a = 0; a < R; ++a) {
                const double v = fabs(sh_g[a]);
                m = (v > m || v != v) ? v : m;
            }
            sh_sc[2] = m;
        }
        __syncthreads();
        const double m = sh_sc[2];
        __syncthreads();
        return m;
    };

    for (int a = tid; a < Rp; a += kBlock) {
        sh_th[a] = 0.0;
        sh_tr[a] = 0.0;
    }
    __syncthreads();
    double F = pass(sh_th, true);
    const double F0 = F;
    double gn = gmax();
    const double g0 = gn;
    int n_iter = 0;
    while (n_iter < A.max_iter && !(gn <= A.tol * g0)) {
        // H = L L' in place (right-looking); a pivot that is not positive ends the column
        bool ok = true;
        for (int j = 0; j < R; ++j) {
            const int jj = j * (j + 1) / 2 + j;
            const double piv = sh_H[jj];
            __syncthreads();
            if (!(piv > 0.0)) {
                ok = false;
                break;
            }
            const double dj = sqrt(piv);
            if (tid == 0) sh_H[jj] = dj;
            for (int i = j + 1 + tid; i < R; i += kBlock) sh_H[i * (i + 1) / 2 + j] /= dj;
            __syncthreads();
            const int m = R - j - 1;
            for (int e = tid; e < m * (m + 1) / 2; e += kBlock) {
                int a, b;
                foldin_tri(e, a, b);
                a += j + 1;
                b += j + 1;
                sh_H[a * (a + 1) / 2 + b] -= sh_H[a * (a + 1) / 2 + j] * sh_H[b * (b + 1) / 2 + j];
            }
            __syncthreads();
        }
        if (!ok) break;
        // L u = -g, L' s = u
        if (tid < R) sh_s[tid] = -sh_g[tid];
        __syncthreads();
        for (int j = 0; j < R; ++j) {
            if (tid == 0) sh_s[j] /= sh_H[j * (j + 1) / 2 + j];
            __syncthreads();
            const double uj = sh_s[j];
            for (int i = j + 1 + tid; i < R; i += kBlock) sh_s[i] -= sh_H[i * (i + 1) / 2 + j] * uj;
            __syncthreads();
        }
        for (int j = R - 1; j >= 0; --j) {
            if (tid == 0) sh_s[j] /= sh_H[j * (j + 1) / 2 + j];
            __syncthreads();
            const double sj = sh_s[j];
            for (int i = tid; i < j; i += kBlock) sh_s[i] -= sh_H[j * (j + 1) / 2 + i] * sj;
            __syncthreads();
        }
        if (tid == 0) {
            double sl = 0.0;
            for (int a = 0; a < R; ++a) sl += sh_g[a] * sh_s[a];
            sh_sc[2] = sl;
        }
        __syncthreads();
        const double slope = sh_sc[2];
        __syncthreads();
        // Armijo backtracking on F_j.  F is a sum of rows + R non-negative terms added one after
        // the other: two computed values of it are compared up to that sum's rounding bound, so
        // that a step whose decrease is below it is not mistaken for a stall.
        const double slack = (double)(r1 - r0 + R + 2) * 0x1p-52 * F;
        double t = 1.0, Ft = F;
        bool accepted = false;
        for (int hv = 0; hv <= kFoldinHalvings; ++hv) {
            if (tid < R) sh_tr[tid] = sh_th[tid] + t * sh_s[tid];
            __syncthreads();
            Ft = pass(sh_tr, false);
            if (Ft <= F + kFoldinArmijo * t * slope + slack) {
                accepted = true;
                break;
            }
            t *= 0.5;
        }
        if (!accepted) break;  // stalled: the column ends here
        if (tid < R) sh_th[tid] = sh_tr[tid];
        __syncthreads();
        ++n_iter;
        F = pass(sh_th, true);
        gn = gmax();
    }
    for (int a = tid; a < R; a += kBlock) A.theta[(size_t)col * R + a] = sh_th[a];
    if (tid == 0) {
        A.stat[col * 3 + 0] = gn;
        A.stat[col * 3 + 1] = F0;
        A.stat[col * 3 + 2] = F;
        A.it[col * 2 + 0] = n_iter;
        A.it[col * 2 + 1] = (gn <= A.tol * g0) ? 1 : 0;
    }
}

}  // namespace spfm
