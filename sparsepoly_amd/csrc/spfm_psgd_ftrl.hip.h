// spfm_psgd_ftrl.hip.h -- FTRL-Proximal steps of the minibatch unit
// Part of the gfx950 device code of the sparse-FM solvers; see spfm_psgd.hip.h for the unit.
//
//   psgd_update_ftrl_kernel  the update that follows a minibatch's gradient in FTRL mode
//                            (spfm_psgd_set_ftrl): per-column accumulators n, the dual average z,
//                            the closed form of p from z -- and nothing at all for a column whose
//                            gradient is zero
//   psgd_ftrl_init_kernel    the starting z of a handle: the z whose closed form at n = 0 gives
//                            back the parameters as they stand
//
// The rule (McMahan et al., "Ad click prediction: a view from the trenches", per-coordinate FTRL-
// Proximal with L1 and L2, lazy form), with one accumulator per (order, column) so that the step is
// one scalar inside every group l1 and l21 prox over:
//   g = grad_P[o, j, :] / B,  g2 = |g|^2;  g2 == 0: the column is left exactly as it is
//   sigma = (sqrt(n + g2) - sqrt(n)) / eta;  z += g - sigma * p;  n += g2
//   denom = (G0 + sqrt(n)) / eta + beta
//   l1 : p = -soft(z, gamma) / denom          l21: p = -max(0, 1 - gamma / |z|) z / denom
// and for w with (z_w, n_w), alpha in beta's place and no sparse term.
//
// Decomposition as psgd_update_kernel: one L-lane group per (order, column), lane = component,
// kPsgdMaxC chunks for k > L, a grid-stride loop over the columns, the w loop on top.  The memory
// side is ordered around the lazy test: a column's grad_P chunks are loaded first (all of them in
// flight together, <= 4 doubles per lane), one group_sum gives g2, and on the group-uniform branch
// g2 == 0 the group goes on to its next column -- 8k bytes read, nothing written; grad_P is zero
// already.  A touched column then loads n, z, p and stores z, p, n and the zeros of grad_P:
// 48k + 16 bytes.  Every lane forms the column's scalars itself (two square roots, 1/denom and
// for l21 gamma / |z|): the lanes of a wave run in lockstep, so one lane computing them would cost
// the same instructions plus the shuffles that hand the results round.  1/B and 1/eta are formed
// once per thread.  No block-level synchronisation, no LDS, plain vector stores, no atomics; the
// trip counts around the shuffles (chunks, columns of a group) are group-uniform.
#pragma once
#include "spfm_psgd.hip.h"

namespace spfm {

// `b`: the minibatch's scalars (B, eta_P, eta_w, alpha, beta, gamma, g0); table-driven (graph
// replay), sched[idx[1]] replaces it, so no recorded argument can go stale between two epochs.
template <int L>
__global__ __launch_bounds__(kBlock) void psgd_update_ftrl_kernel(
    double* __restrict__ Pt, double* __restrict__ grad_P, double* __restrict__ w,
    double* __restrict__ grad_w, double* __restrict__ z_P, double* __restrict__ n_P,
    double* __restrict__ z_w, double* __restrict__ n_w, int n_orders, int k, int d, int reg,
    int fit_linear, PsgdBatch b, const PsgdBatch* __restrict__ sched, int* __restrict__ idx) {
    constexpr int gpb = kBlock / L;
    if (sched) {  // table-driven (graph replay): batch idx[1], then hand idx[0] on
        const int bi = idx[1];
        b = sched[bi];
        if (blockIdx.x == 0 && threadIdx.x == 0) idx[0] = bi + 1;
    }
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    const int C = (k + L - 1) / L;
    const double rB = 1.0 / (double)b.B;  // (the f64 divisions of this pass: two per thread here,
                                          // one per touched column below, one more for l21)
    if (fit_linear) {
        const double reta = 1.0 / b.eta_w;
        for (int j = blockIdx.x * kBlock + threadIdx.x; j < d; j += gridDim.x * kBlock) {
            const double g = grad_w[j] * rB;
            if (g * g == 0.0) continue;  // untouched: w[j], z_w[j], n_w[j] stay what they are
            grad_w[j] = 0.0;
            const double n0 = n_w[j], n1 = n0 + g * g;
            const double s1 = sqrt(n1);
            const double wj = w[j];
            const double z = z_w[j] + g - (s1 - sqrt(n0)) * reta * wj;
            n_w[j] = n1;
            z_w[j] = z;
            w[j] = -z / ((b.g0 + s1) * reta + b.alpha);
        }
    }
    const double reta = 1.0 / b.eta_P;
    for (int o = 0; o < n_orders; ++o) {
        for (int j = blockIdx.x * gpb + grp; j < d; j += gridDim.x * gpb) {
            const size_t col = (size_t)o * d + j, base = col * k;
            double g[kPsgdMaxC];
            double q = 0.0;
#pragma unroll
            for (int c = 0; c < kPsgdMaxC; ++c) {
                const int s = c * L + ln;
                g[c] = (c < C && s < k) ? grad_P[base + s] * rB : 0.0;
                q += g[c] * g[c];
            }
            const double g2 = group_sum(q, L);
            if (g2 == 0.0) continue;  // the lazy property: no further load, no store
            const double n0 = n_P[col];
            double z[kPsgdMaxC], p[kPsgdMaxC];
#pragma unroll
            for (int c = 0; c < kPsgdMaxC; ++c) {
                const int s = c * L + ln;
                const bool in = c < C && s < k;
                z[c] = in ? z_P[base + s] : 0.0;
                p[c] = in ? Pt[base + s] : 0.0;
            }
            const double n1 = n0 + g2;
            const double s1 = sqrt(n1);
            const double sigma = (s1 - sqrt(n0)) * reta;
            const double rden = 1.0 / ((b.g0 + s1) * reta + b.beta);
            q = 0.0;
#pragma unroll
            for (int c = 0; c < kPsgdMaxC; ++c) {
                z[c] = z[c] + g[c] - sigma * p[c];
                q += z[c] * z[c];
            }
            if (reg == REG_L1) {
#pragma unroll
                for (int c = 0; c < kPsgdMaxC; ++c) p[c] = -soft_thr(z[c], b.gamma) * rden;
            } else if (reg == REG_L21) {
                const double nz = sqrt(group_sum(q, L));
                const double f = nz > b.gamma ? (1.0 - b.gamma / nz) * rden : 0.0;
#pragma unroll
                for (int c = 0; c < kPsgdMaxC; ++c) p[c] = -f * z[c];
            } else {
#pragma unroll
                for (int c = 0; c < kPsgdMaxC; ++c) p[c] = -z[c] * rden;
            }
#pragma unroll
            for (int c = 0; c < kPsgdMaxC; ++c) {
                const int s = c * L + ln;
                if (c < C && s < k) {
                    grad_P[base + s] = 0.0;
                    z_P[base + s] = z[c];
                    Pt[base + s] = p[c];
                }
            }
            if (ln == 0) n_P[col] = n1;
        }
    }
}

// The starting state: n = 0 and the z whose closed form at n = 0 is the handle's (P, w), with
// denom0 = G0 / eta0 + beta:
//   l1 : z = -(p denom0 + sign(p) gamma), 0 for p = 0
//   l21: z = -(denom0 |p_j| + gamma) p_j / |p_j|, 0 for a zero column
//   z_w = -w (G0 / eta0 + alpha)
// (any other regularizer: no sparse term; the epochs refuse it anyway).  Same decomposition as the
// update; one division per column for l21.
template <int L>
__global__ __launch_bounds__(kBlock) void psgd_ftrl_init_kernel(
    const double* __restrict__ Pt, const double* __restrict__ w, double* __restrict__ z_P,
    double* __restrict__ n_P, double* __restrict__ z_w, double* __restrict__ n_w, int n_orders,
    int k, int d, int reg, double g0, double eta0, double alpha, double beta, double gamma) {
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    const int C = (k + L - 1) / L;
    const double den_w = g0 / eta0 + alpha, den_P = g0 / eta0 + beta;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < d; j += gridDim.x * kBlock) {
        z_w[j] = -w[j] * den_w;
        n_w[j] = 0.0;
    }
    for (int o = 0; o < n_orders; ++o) {
        for (int j = blockIdx.x * gpb + grp; j < d; j += gridDim.x * gpb) {
            const size_t col = (size_t)o * d + j, base = col * k;
            double p[kPsgdMaxC];
            double q = 0.0;
#pragma unroll
            for (int c = 0; c < kPsgdMaxC; ++c) {
                const int s = c * L + ln;
                p[c] = (c < C && s < k) ? Pt[base + s] : 0.0;
                q += p[c] * p[c];
            }
            double scale = den_P;  // l21: (denom0 |p| + gamma) / |p|
            if (reg == REG_L21) {
                const double nr = sqrt(group_sum(q, L));
                scale = nr > 0.0 ? (den_P * nr + gamma) / nr : 0.0;
            }
#pragma unroll
            for (int c = 0; c < kPsgdMaxC; ++c) {
                const int s = c * L + ln;
                if (c < C && s < k) {
                    const double sg = (double)((p[c] > 0) - (p[c] < 0));
                    z_P[base + s] = reg == REG_L1 ? -(p[c] * den_P + sg * gamma) : -(p[c] * scale);
                }
            }
            if (ln == 0) n_P[col] = 0.0;
        }
    }
}

}  // namespace spfm
