// spfm_psgd_pairs_det.hip.h -- the deterministic minibatch gradient of the pairwise ranking fit
// (DESIGN.md section 19f).  Part of the gfx950 device code of the sparse-FM solvers; see
// spfm_psgd_pairs.hip.h for the triples and spfm_psgd_det.hip.h for the pointwise route.
//
// psgd_pair_grad_kernel scatters every triple's terms with f64 atomics.  Here the same terms are
// added in a fixed order.  With the minibatch the triples at positions [pos, pos + B):
//   grad_P[o, j, s] = sum over the triples r of the batch, ascending, and inside a triple in the
//                     order anchor, plus, minus, of
//                       anchor   dL lams_s (D+_j - D-_j)     j stored in the anchor row
//                       plus    +dL lams_s  D+_j             j stored in c+
//                       minus   -dL lams_s  D-_j             j stored in c-
//   grad_w[j]       likewise of +dL z+_j (plus) and -dL z-_j (minus); anchor columns get no term.
// Every term is formed by the expressions of pair_grad / pair_margin_out: dl (D+ - D-) with
// dl = dL lams_s, D of a row the entry is not part of being the recurrence run with x = 0.  A
// column stored in c+ and in c- of one triple contributes its two terms in that order.  dL carries
// the triple's weight where the atomic route multiplies it (dL = weights[r] * dloss); a triple of
// weight 0 KEEPS its records and contributes exact-zero terms (its dL and loss are set to exact
// 0: the values of the atomic route, which skips the triple, as long as its DP values are
// finite), so the plan and the shape of every sum are functions of the triple list and
// batch_size alone -- never of the weights, the grid, or graph replay against eager launches.
// A (minibatch, column) run longer than kDetSeg records is cut into pieces of kDetSeg; the pieces
// start from zero and are added in ascending piece order (spfm_psgd_det.hip.h), so the shape of
// a sum depends on the run's length alone.
//
// Per epoch a plan enumerates the stored entries of the three rows of every triple -- by
// position, inside a triple anchor, plus, minus --, sorts them stably by
// (position / batch_size) * d + column, and keeps per record {r, role, x}: r the triple's place
// in its minibatch and the role (2 bits) in one word.  Per minibatch two kernels run on a fixed
// grid-stride grid:
//   psgd_pair_rowstate_kernel  the front half of psgd_pair_grad_kernel (one L-lane group per
//                              triple): the context's DP once, continued over c+ and, from a
//                              copy, over c-; margin, dL_r (weighted), loss_row; both DP arrays
//                              go to state[B][2][n_orders][degree - 1][k]; no gradient
//   psgd_pair_colgrad_kernel   one L-lane group per run (lane = component): records L at a time,
//                              broadcast by group shuffles, the state loads of kDetU records in
//                              flight, D+ / D- rebuilt by the downward recurrence, one register
//                              accumulator, one plain store per (o, j, s) and per w_j
// No float atomics anywhere; update and Michelot kernels are those of spfm_psgd.hip.h.
#pragma once
#include "spfm_psgd_det.hip.h"
#include "spfm_psgd_pairs.hip.h"

namespace spfm {

constexpr int kPairRoleBits = 2;  // record word = (r << 2) | role
constexpr int kRoleAnchor = 0, kRolePlus = 1, kRoleMinus = 2;

// The plan as the gradient kernels see it: DetPlan's tables with rec = (r << 2) | role.
struct PairDetPlan {
    const int32_t* bseg_ptr;
    const int32_t* seg_ptr;
    const int32_t* seg_col;
    const uint32_t* rec;
};

// ------------------------------------------------------------------ the plan's kernels
// (det_seg_kernel, det_longest_kernel and det_differ_kernel of the pointwise plan are reused)
// len[q] = stored entries of the three rows of the triple at position q
static __global__ __launch_bounds__(kBlock) void pair_det_len_kernel(
    const int32_t* __restrict__ triples, const int64_t* __restrict__ rptr, int64_t m,
    int64_t* __restrict__ len) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= m) return;
    int64_t s = 0;
    for (int a = 0; a < 3; ++a) {
        const int i = triples[3 * q + a];
        s += rptr[i + 1] - rptr[i];
    }
    len[q] = s;
}

// entry u of the concatenation anchor | plus | minus of the triple at position q -> its place in
// the CSR arrays and its role
struct PairEntry {
    int64_t l[3];
    int64_t n0, n1, tot;
    __device__ __forceinline__ PairEntry(const int32_t* __restrict__ triples,
                                         const int64_t* __restrict__ rptr, int64_t q) {
        int64_t cnt[3];
        for (int a = 0; a < 3; ++a) {
            const int i = triples[3 * q + a];
            l[a] = rptr[i];
            cnt[a] = rptr[i + 1] - l[a];
        }
        n0 = cnt[0];
        n1 = cnt[0] + cnt[1];
        tot = n1 + cnt[2];
    }
    __device__ __forceinline__ int role(int64_t u) const {
        return u < n0 ? kRoleAnchor : u < n1 ? kRolePlus : kRoleMinus;
    }
    __device__ __forceinline__ int64_t at(int64_t u) const {
        return u < n0 ? l[0] + u : u < n1 ? l[1] + (u - n0) : l[2] + (u - n1);
    }
};

// one record per stored entry, in position order and inside a triple in role order (16 lanes per
// position): entry m = qoff[q] + u gets key (q / batch_size) * d + column, value m, ent_q[m] = q
static __global__ __launch_bounds__(kBlock) void pair_det_enum_kernel(
    const int32_t* __restrict__ triples, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const int64_t* __restrict__ qoff, int64_t m,
    int64_t batch_size, int d, uint64_t* __restrict__ key, uint32_t* __restrict__ val,
    int32_t* __restrict__ ent_q) {
    const int64_t q = (int64_t)blockIdx.x * (kBlock / 16) + threadIdx.x / 16;
    if (q >= m) return;
    const PairEntry pe(triples, rptr, q);
    const int64_t base = qoff[q];
    const uint64_t kb = (uint64_t)(q / batch_size) * (uint64_t)d;
    for (int64_t u = threadIdx.x % 16; u < pe.tot; u += 16) {
        key[base + u] = kb + (uint64_t)ridx[pe.at(u)];
        val[base + u] = (uint32_t)(base + u);
        ent_q[base + u] = (int32_t)q;
    }
}

// behind the sort: the records in sorted order and the head flag of every (minibatch, column) run
template <typename T>
__global__ __launch_bounds__(kBlock) void pair_det_head_kernel(
    const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
    const int32_t* __restrict__ ent_q, const int32_t* __restrict__ triples,
    const int64_t* __restrict__ rptr, const T* __restrict__ rval,
    const int64_t* __restrict__ qoff, int64_t N, int64_t batch_size, uint32_t* __restrict__ rec,
    T* __restrict__ rec_x, int32_t* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= N) return;
    const int64_t e = val[t];
    const int64_t q = ent_q[e];
    const PairEntry pe(triples, rptr, q);
    const int64_t u = e - qoff[q];
    rec[t] = ((uint32_t)(q % batch_size) << kPairRoleBits) | (uint32_t)pe.role(u);
    rec_x[t] = rval[pe.at(u)];
    flag[t] = (t == 0 || key[t] != key[t - 1]) ? 1 : 0;
}

// ------------------------------------------------------------------ the gradient kernels
// The register-resident shape of one triple at degree DEG (one order, k <= L, the three rows fit
// one chunk together): pair_keep's front half.  The packed chunk's P loads are issued back to
// back; the margin's share goes into m, the DP values a+^t / a-^t, t = 1 .. DEG - 1, to st / st +
// side (st: the triple's state at this lane's component).
template <typename T, int L, int DEG>
__device__ __forceinline__ void pair_state_keep(int64_t l0, int nb, int64_t l1, int np, int64_t l2,
                                                int nm, int ln, int k,
                                                const int32_t* __restrict__ ridx,
                                                const T* __restrict__ rval,
                                                const double* __restrict__ Pt,
                                                const double* __restrict__ lams, double& m,
                                                double* __restrict__ st, size_t side) {
    const bool act = ln < k;
    PsgdChunk<T, L> ch;
    PairX<L> px;
    double ap[kMaxDegree + 1], am[kMaxDegree + 1];
    pair_load_packed(ch, px, l0, nb, l1, np, l2, nm, ln, ridx, rval);
    ch.load_p(Pt + (act ? ln : 0), k, act);
    psgd_a_init(ap);
    psgd_a_init(am);
    pair_dp_packed<T, L, DEG>(ch, px, ap, am);
    if (!act) return;
    m += lams[ln] * (ap[DEG] - am[DEG]);
#pragma unroll
    for (int t = 1; t < DEG; ++t) {
        st[(size_t)(t - 1) * k] = ap[t];
        st[side + (size_t)(t - 1) * k] = am[t];
    }
}

// The front half of psgd_pair_grad_kernel for the triples of one minibatch, on a fixed grid (the
// triples are walked with a grid stride, whole groups at a time): dLrow[r] (times weights[r] with
// WT), loss_row[r], and the DP values of both summed rows of triple r in
//   state[(((r * 2 + h) * n_orders + o) * (degree - 1) + (t - 1)) * k + s] = a_s^t,
//   h = 0: x_b + z_c+, h = 1: x_b + z_c-,  t = 1 .. degree - o - 1   (a^0 = 1 is not stored)
// No gradient is written.  A triple of weight 0 is computed like any other; its dL and loss are
// set to exact 0.
template <typename T, int L, bool WT>
__global__ __launch_bounds__(kBlock) void psgd_pair_rowstate_kernel(
    const int32_t* __restrict__ triples, int B, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const double* __restrict__ Pt,
    const double* __restrict__ w, const double* __restrict__ lams, int n_orders, int k, int d,
    int degree, int loss, double* __restrict__ dLrow, double* __restrict__ state,
    double* __restrict__ loss_row, const PsgdBatch* __restrict__ sched, int* __restrict__ idx,
    const double* __restrict__ weights) {
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    if (sched) {
        long long pos;
        psgd_table_batch(sched, idx, B, pos);
        triples += 3 * pos;
        loss_row += pos;
        if (WT) weights += pos;
    }
    const int C = (k + L - 1) / L;
    const int nst = degree - 1;
    const size_t side = (size_t)n_orders * nst * k;
    for (int r = blockIdx.x * gpb + grp; r < B; r += gridDim.x * gpb) {  // whole groups
        const int ib = triples[3 * (size_t)r], ip = triples[3 * (size_t)r + 1],
                  im = triples[3 * (size_t)r + 2];
        const int64_t l0 = rptr[ib], h0 = rptr[ib + 1];  // the context's entries
        const int64_t l1 = rptr[ip], h1 = rptr[ip + 1];  // c+
        const int64_t l2 = rptr[im], h2 = rptr[im + 1];  // c-
        double* st = state + (size_t)r * 2 * side;
        // the margin, by the expressions of psgd_pair_grad_kernel
        double m = 0.0;
        for (int64_t e = l1 + ln; e < h1; e += L) m += (double)rval[e] * w[ridx[e]];
        for (int64_t e = l2 + ln; e < h2; e += L) m -= (double)rval[e] * w[ridx[e]];
        if (n_orders == 1 && C == 1 && (h0 - l0) + (h1 - l1) + (h2 - l2) <= kPsgdRC) {
#define SPFM_PAIR_STATE(DEG)                                                                     \
    case DEG:                                                                                    \
        pair_state_keep<T, L, DEG>(l0, (int)(h0 - l0), l1, (int)(h1 - l1), l2, (int)(h2 - l2),   \
                                   ln, k, ridx, rval, Pt, lams, m, st + (ln < k ? ln : 0), side); \
        break
            switch (degree) {
                SPFM_PAIR_STATE(2);
                SPFM_PAIR_STATE(3);
                SPFM_PAIR_STATE(4);
                SPFM_PAIR_STATE(5);
                SPFM_PAIR_STATE(6);
            }
#undef SPFM_PAIR_STATE
        } else {
            PsgdChunk<T, L> ch;
            double ap[kMaxDegree + 1], am[kMaxDegree + 1];
            for (int o = 0; o < n_orders; ++o) {
                const int deg = degree - o;
                for (int c = 0; c < C; ++c) {
                    const int s = c * L + ln;
                    const bool act = s < k;
                    pair_dp_rows(ch, l0, h0, l1, h1, l2, h2, ln, ridx, rval,
                                 Pt + (size_t)o * d * k + (act ? s : 0), k, act, deg, ap, am);
                    if (act) {
                        m += lams[s] * pair_top_diff(ap, am, deg);
                        double* so = st + (size_t)o * nst * k + s;
#pragma unroll
                        for (int t = 1; t < kMaxDegree; ++t)
                            if (t < deg) {
                                so[(size_t)(t - 1) * k] = ap[t];
                                so[side + (size_t)(t - 1) * k] = am[t];
                            }
                    }
                }
            }
        }
        m = group_sum(m, L);
        double ls = loss_dev(loss, m, 1.0), dL = dloss_dev(loss, m, 1.0);
        if (WT) {  // weight 0: exact zeros, whatever the margin (0 * inf would be NaN)
            const double wt = weights[r];
            ls = wt == 0.0 ? 0.0 : wt * ls;
            dL = wt == 0.0 ? 0.0 : wt * dL;
        }
        if (ln == 0) {
            loss_row[r] = ls;
            dLrow[r] = dL;
        }
    }
}

// The partial sums of the records [e0, e1) (one piece, <= kDetSeg) for one component lane of one
// order, in record order from zero: gp of dl (D+ - D-) and, with `lin` (the one (order, chunk)
// whose lane 0 stores w_j), gw of +-dL x (candidates' records alone; else gw stays 0).
// The records are loaded L at a time, lane-parallel, and broadcast with group shuffles, so the
// dependent state loads of kDetU records are issued back to back: an anchor record reads both
// states, a plus record a+ alone, a minus record a- alone (the other enters as x = 0, whose D is
// 0, as in pair_grad).  `st`: the state of triple 0, h = 0, for this (order, lane).
template <typename T, int L>
__device__ __forceinline__ void pair_det_piece(int e0, int e1, int ln,
                                               const uint32_t* __restrict__ rec,
                                               const T* __restrict__ rec_x,
                                               const double* __restrict__ dLrow,
                                               const double* __restrict__ st, size_t side,
                                               size_t rstride, int k, int deg, double lam, double p,
                                               bool act, bool lin, double& gp, double& gw) {
    gp = 0.0;
    gw = 0.0;
    for (int tb = e0; tb < e1; tb += L) {
        const int e = tb + ln;
        const bool in = e < e1;
        const int wl = in ? (int)rec[e] : 0;
        const double xl = in ? (double)rec_x[e] : 0.0;
        const double dl = in ? dLrow[(uint32_t)wl >> kPairRoleBits] : 0.0;
        const int cnt = (e1 - tb < L) ? (e1 - tb) : L;
#pragma unroll
        for (int sb = 0; sb < L; sb += kDetU) {
            if (sb >= cnt) break;  // (the same for every lane of the group)
            double a[kDetU][2][kMaxDegree - 1];
#pragma unroll
            for (int u = 0; u < kDetU; ++u) {
                const uint32_t wd = (uint32_t)__shfl(wl, sb + u, L);
                const int role = (int)(wd & 3u);
                const double* sr = st + (size_t)(wd >> kPairRoleBits) * rstride;
                const bool live = act && sb + u < cnt;
#pragma unroll
                for (int t = 1; t < kMaxDegree; ++t) {
                    a[u][0][t - 1] =
                        (live && role != kRoleMinus && t < deg) ? sr[(size_t)(t - 1) * k] : 0.0;
                    a[u][1][t - 1] = (live && role != kRolePlus && t < deg)
                                         ? sr[side + (size_t)(t - 1) * k]
                                         : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < kDetU; ++u) {
                const int role = __shfl(wl, sb + u, L) & 3;
                const double x = __shfl(xl, sb + u, L);
                const double dL = __shfl(dl, sb + u, L);
                const double xp = role != kRoleMinus ? x : 0.0;
                const double xm = role != kRolePlus ? x : 0.0;
                double dp = xp, dm = xm;
#pragma unroll
                for (int t = 1; t < kMaxDegree; ++t)
                    if (t < deg) {
                        dp = xp * (a[u][0][t - 1] - p * dp);
                        dm = xm * (a[u][1][t - 1] - p * dm);
                    }
                if (sb + u < cnt) {
                    gp += (dL * lam) * (dp - dm);
                    if (lin && role == kRolePlus) gw += dL * x;
                    if (lin && role == kRoleMinus) gw += -dL * x;
                }
            }
        }
    }
}

// The runs of one minibatch on a fixed grid: a workgroup walks blocks of kBlock / L consecutive
// runs with a grid stride, one group per run of at most kDetSeg records; the longer runs of the
// block are then taken by all its groups together, a piece each, and folded by group 0 through LDS
// in piece order.  Every thread of the workgroup reads the same bounds, so the barriers are
// reached by all (no early return).  bi: the minibatch (table-driven: idx[0]).
template <typename T, int L>
__global__ __launch_bounds__(kBlock) void psgd_pair_colgrad_kernel(
    PairDetPlan pl, const T* __restrict__ rec_x, int bi, const double* __restrict__ Pt,
    const double* __restrict__ lams, const double* __restrict__ dLrow,
    const double* __restrict__ state, int n_orders, int k, int d, int degree, int fit_linear,
    double* __restrict__ grad_P, double* __restrict__ grad_w, const int* __restrict__ idx) {
    constexpr int gpb = kBlock / L;
    __shared__ double red[gpb][L + 1];  // [g][L]: the piece's gw
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    if (idx) bi = idx[0];
    const int slo = pl.bseg_ptr[bi], shi = pl.bseg_ptr[bi + 1];
    const int C = (k + L - 1) / L;
    const int nst = degree - 1;
    const size_t side = (size_t)n_orders * nst * k;
    const size_t rstride = 2 * side;
    for (int sb = slo + blockIdx.x * gpb; sb < shi; sb += gridDim.x * gpb) {
        const int s = sb + grp;
        if (s < shi) {
            const int e0 = pl.seg_ptr[s], e1 = pl.seg_ptr[s + 1];
            if (e1 - e0 <= kDetSeg) {
                const int j = pl.seg_col[s];
                for (int o = 0; o < n_orders; ++o)
                    for (int c = 0; c < C; ++c) {
                        const int cs = c * L + ln;
                        const bool act = cs < k;
                        const size_t at = ((size_t)o * d + j) * k + (act ? cs : 0);
                        const bool lin = fit_linear && o == 0 && c == 0;
                        double gp, gw;
                        pair_det_piece<T, L>(e0, e1, ln, pl.rec, rec_x, dLrow,
                                             state + (size_t)o * nst * k + (act ? cs : 0), side,
                                             rstride, k, degree - o, act ? lams[cs] : 0.0,
                                             act ? Pt[at] : 0.0, act, lin, gp, gw);
                        if (act) grad_P[at] = gp;
                        if (lin && ln == 0) grad_w[j] = gw;
                    }
            }
        }
        // the long runs of this block
        for (int g2 = 0; g2 < gpb && sb + g2 < shi; ++g2) {
            const int e0 = pl.seg_ptr[sb + g2], e1 = pl.seg_ptr[sb + g2 + 1];
            if (e1 - e0 <= kDetSeg) continue;
            const int j = pl.seg_col[sb + g2];
            const int npc = (e1 - e0 + kDetSeg - 1) / kDetSeg;
            for (int o = 0; o < n_orders; ++o)
                for (int c = 0; c < C; ++c) {
                    const int cs = c * L + ln;
                    const bool act = cs < k;
                    const size_t at = ((size_t)o * d + j) * k + (act ? cs : 0);
                    const double lam = act ? lams[cs] : 0.0, p = act ? Pt[at] : 0.0;
                    const bool lin = fit_linear && o == 0 && c == 0;
                    double tp = 0.0, tw = 0.0;
                    for (int p0 = 0; p0 < npc; p0 += gpb) {
                        const int pc = p0 + grp;
                        double gp = 0.0, gw = 0.0;
                        if (pc < npc) {
                            const int f0 = e0 + pc * kDetSeg;
                            pair_det_piece<T, L>(f0, (e1 - f0 < kDetSeg) ? e1 : f0 + kDetSeg, ln,
                                                 pl.rec, rec_x, dLrow,
                                                 state + (size_t)o * nst * k + (act ? cs : 0), side,
                                                 rstride, k, degree - o, lam, p, act, lin, gp,
                                                 gw);
                        }
                        __syncthreads();  // group 0 has read the round before
                        red[grp][ln] = gp;
                        if (lin && ln == 0) red[grp][L] = gw;
                        __syncthreads();
                        if (grp == 0)
                            for (int g = 0; g < gpb && p0 + g < npc; ++g) {
                                tp += red[g][ln];
                                if (lin) tw += red[g][L];
                            }
                    }
                    if (grp == 0 && act) grad_P[at] = tp;
                    if (grp == 0 && lin && ln == 0) grad_w[j] = tw;
                }
        }
    }
}

}  // namespace spfm
