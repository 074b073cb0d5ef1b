// spfm_psgd_lists.hip.h -- listwise ranking gradient of the minibatch solver
// Part of the gfx950 device code of the sparse-FM solvers; see spfm_psgd_pairs.hip.h.
//
// A training item is a LIST: a positive (b, c_0) and its M negatives c_1..c_M, stored as the M
// grouped triples (b, c_0, c_i) the sampler writes (rows qM .. qM+M-1 of the triple list share
// anchor and plus).  With the scores s_i = s(b, c_i) of spfm_psgd_sample.hip.h,
//   'softmax'   L = -s_0 + log sum_{i=0..M} exp(s_i)          coef_i = pi_i - [i == 0]
//   'list'      L = (1/M) sum_{i>=1} loss(s_0 - s_i, +1)      coef_i = -dloss_i / M,
//                                                            coef_0 = -sum_{i>=1} coef_i
// and coef_i = dL/ds_i.  PsgdChunk::grad's recurrence dprev_1 = x, dprev_{t+1} = x (a[t] - p
// dprev_t) is linear in the DP array a[0..deg-1] with coefficients that depend on the entry
// (x, p) alone, so for a context column j
//   sum_i coef_i D_j(a^(i)) = D'_j(abar),   abar[t] = sum_i coef_i a^(i)[t],
// D' the same recurrence started at dprev_1 = x abar[0].  Both losses have sum_i coef_i = 0, so
// abar[0] is taken as exactly 0: ONE gradient pass and ONE atomic per context column whatever M
// is, and the context's linear term and its grad_w are never formed.  The candidates' own columns
// get coef_i lams_s D_j(a^(i)) and coef_i x each (a candidate that appears twice counts twice).
// What follows the gradient (psgd_update_kernel, the psgd_mich_* passes) is the pointwise
// solver's, unchanged; the items psgd_batches_tl counts are lists.
#pragma once
#include "spfm_psgd_sample.hip.h"

namespace spfm {

constexpr int kListMaxNeg = 63;  // SPFM_LIST_MAX_NEG: M + 1 scores in 64 / L registers per lane
constexpr int kListSoftmax = 0;  // SPFM_LIST_SOFTMAX
constexpr int kListPairMean = 1;  // SPFM_LIST_PAIRMEAN

__device__ __forceinline__ double group_max(double v, int width) {
    for (int m = width >> 1; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, kWave));
    return v;
}

// One value per candidate of a list (M + 1 <= 64), spread over the L lanes of the group: lane ln
// holds those whose index is congruent to ln modulo L.  Stored and read by selection among the
// VALUES v[0..NS): an indexed element would move the array out of the registers.
template <int L>
struct ListVals {
    static constexpr int NS = 64 / L;
    double v[NS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int t = 0; t < NS; ++t) v[t] = 0.0;
    }
    __device__ __forceinline__ void put(int i, double s, int ln) {  // i: uniform in the group
#pragma unroll
        for (int t = 0; t < NS; ++t)
            if (i == t * L + ln) v[t] = s;
    }
    __device__ __forceinline__ double get(int i) const {  // i: uniform in the group
        double sel = v[0];
#pragma unroll
        for (int t = 1; t < NS; ++t)
            if (i / L == t) sel = v[t];
        return __shfl(sel, i % L, L);
    }
};

// Up to kSampleNF candidates of one list side by side: candidate i0 + u in slot u (i = 0: the
// plus of the list's first triple; i >= 1: the minus of triple i - 1).  Slots past M are empty
// rows.  The same in every lane of the group.
struct ListCands {
    int64_t lo[kSampleNF];
    int len[kSampleNF];
    int maxlen;
    __device__ __forceinline__ void load(const int32_t* __restrict__ trow, int i0, int M,
                                         const int64_t* __restrict__ rptr) {
        maxlen = 0;
#pragma unroll
        for (int u = 0; u < kSampleNF; ++u) {
            const int i = i0 + u;
            const bool on = i <= M;
            const int c = !on ? 0 : (i == 0 ? trow[1] : trow[3 * (size_t)(i - 1) + 2]);
            lo[u] = on ? rptr[c] : 0;
            len[u] = on ? (int)(rptr[c + 1] - lo[u]) : 0;
            maxlen = len[u] > maxlen ? len[u] : maxlen;
        }
    }
};

// ac[u] = a continued over the entries of candidate u, one (order, component chunk): the loop of
// psgd_pair_sample_kernel -- rolled over the candidates' own short rows, every lane reads the
// same entry (no shuffle), trip count uniform within the group.  LIN: lin[u] += <w, z_u>.
template <typename T, bool LIN>
__device__ __forceinline__ void list_continue(const ListCands& lc, const double* a,
                                              double (*ac)[kMaxDegree + 1],
                                              const int32_t* __restrict__ ridx,
                                              const T* __restrict__ rval,
                                              const double* __restrict__ Pcol, int k, int deg,
                                              const double* __restrict__ w, double* lin) {
#pragma unroll
    for (int u = 0; u < kSampleNF; ++u)
#pragma unroll
        for (int t = 0; t <= kMaxDegree; ++t) ac[u][t] = a[t];
    for (int e = 0; e < lc.maxlen; ++e) {
#pragma unroll
        for (int u = 0; u < kSampleNF; ++u) {
            const bool in = e < lc.len[u];
            const int64_t pe = lc.lo[u] + (in ? e : 0);
            const int j = in ? ridx[pe] : 0;
            const double x = in ? (double)rval[pe] : 0.0;  // 0 past the row: a no-op
            const double p = Pcol[(size_t)j * k];
            if (LIN) lin[u] += x * w[j];
#pragma unroll
            for (int t = kMaxDegree; t >= 1; --t)
                if (t <= deg) ac[u][t] += ac[u][t - 1] * x * p;
        }
    }
}

// The candidates' own part of the gradient for one (order, component chunk): per entry of
// candidate u, cl[u] D_j(ac[u]) to grad_P (cl = coef lams_s, 0 in an idle lane) and, with `lin`
// (once per list: the first order and chunk), cf[u] x to grad_w from the group's first lane.
template <typename T>
__device__ __forceinline__ void list_cand_grad(const ListCands& lc,
                                               double (*ac)[kMaxDegree + 1], const double* cl,
                                               const double* cf,
                                               const int32_t* __restrict__ ridx,
                                               const T* __restrict__ rval,
                                               const double* __restrict__ Pcol,
                                               double* __restrict__ Gcol, int k, int deg, bool act,
                                               bool lin, int ln, double* __restrict__ grad_w) {
    for (int e = 0; e < lc.maxlen; ++e) {
#pragma unroll
        for (int u = 0; u < kSampleNF; ++u) {
            const bool in = e < lc.len[u];
            const int64_t pe = lc.lo[u] + (in ? e : 0);
            const int j = in ? ridx[pe] : 0;
            const double x = in ? (double)rval[pe] : 0.0;
            const double p = Pcol[(size_t)j * k];
            double dprev = x;
#pragma unroll
            for (int t = 1; t < kMaxDegree; ++t)
                if (t < deg) dprev = x * (ac[u][t] - p * dprev);
            if (act && in) unsafeAtomicAdd(&Gcol[(size_t)j * k], cl[u] * dprev);
            if (lin && in && ln == 0) unsafeAtomicAdd(&grad_w[j], cf[u] * x);
        }
    }
}

// The scores' way out: the list's loss, the coefficients dL/ds_i in the layout of the scores
// (EVAL: none, and the 0/1 flag s_0 > max_{i>=1} s_i instead).  f64 throughout; the softmax is a
// max-subtracted log-sum-exp.
template <int L, bool EVAL>
__device__ __forceinline__ void list_coefs(const ListVals<L>& sc, ListVals<L>& cf, int M,
                                           int list_loss, int loss, int ln, double* loss_out,
                                           int* first_out) {
    constexpr int NS = ListVals<L>::NS;
    const double s0 = __shfl(sc.v[0], 0, L);
    double mx = -INFINITY, mxn = -INFINITY;  // over all candidates; over the negatives
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int i = t * L + ln;
        if (i <= M) mx = fmax(mx, sc.v[t]);
        if (i >= 1 && i <= M) mxn = fmax(mxn, sc.v[t]);
    }
    if (EVAL) *first_out = s0 > group_max(mxn, L) ? 1 : 0;
    cf.clear();
    if (list_loss == kListSoftmax) {
        mx = group_max(mx, L);
        double ex[NS], z = 0.0;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            ex[t] = (t * L + ln <= M) ? exp(sc.v[t] - mx) : 0.0;
            z += ex[t];
        }
        z = group_sum(z, L);
        *loss_out = (mx - s0) + log(z);
#pragma unroll
        for (int t = 0; t < NS; ++t) cf.v[t] = ex[t] / z - ((t == 0 && ln == 0) ? 1.0 : 0.0);
        return;
    }
    double ls = 0.0, c0 = 0.0;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int i = t * L + ln;
        if (i >= 1 && i <= M) {
            ls += loss_dev(loss, s0 - sc.v[t], 1.0);
            cf.v[t] = -dloss_dev(loss, s0 - sc.v[t], 1.0) / (double)M;
            c0 -= cf.v[t];
        }
    }
    *loss_out = group_sum(ls, L) / (double)M;
    c0 = group_sum(c0, L);
    if (ln == 0) cf.v[0] = c0;
}

// One list in one of the kernel's two forms, each with its own state and its own end.  KEEP: one
// order, k <= L and a context of one chunk -- the context's chunk (entries and P values) and its
// DP array stay in registers from the scores to the gradient.  Otherwise the context's DP is
// recomputed per (order, component chunk), for every batch of candidates in the scores and once
// in the gradient, and its gradient runs in chunks of kPsgdRC.
template <typename T, int L, bool EVAL, bool KEEP>
__device__ __forceinline__ void list_run(
    const int32_t* __restrict__ trow, size_t at, int64_t l0, int64_t h0, int M, int list_loss,
    int ln, const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const T* __restrict__ rval, const double* __restrict__ Pt, const double* __restrict__ w,
    const double* __restrict__ lams, int n_orders, int k, int d, int degree, int loss,
    int fit_linear, double* __restrict__ grad_P, double* __restrict__ grad_w,
    double* __restrict__ loss_row, int* __restrict__ first) {
    constexpr bool keep = KEEP;
    const int C = KEEP ? 1 : (k + L - 1) / L;
    if (KEEP) n_orders = 1;
    PsgdChunk<T, L> ch;
    ListCands lc;
    double a[kMaxDegree + 1], ac[kSampleNF][kMaxDegree + 1];
    if (keep) {
        const bool act = ln < k;
        psgd_a_init(a);
        psgd_row_dp(ch, l0, h0, ln, ridx, rval, Pt + (act ? ln : 0), k, act, degree, a);
    }
    // pass 1: the scores, kSampleNF candidates at a time
    ListVals<L> sc, cf;
    sc.clear();
    for (int i0 = 0; i0 <= M; i0 += kSampleNF) {
        lc.load(trow, i0, M, rptr);
        double part[kSampleNF], lin[kSampleNF];
#pragma unroll
        for (int u = 0; u < kSampleNF; ++u) part[u] = lin[u] = 0.0;
        for (int o = 0; o < n_orders; ++o) {
            const int deg = degree - o;
            for (int c = 0; c < C; ++c) {
                const int s = c * L + ln;
                const bool act = s < k;
                const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
                if (!keep) {
                    psgd_a_init(a);
                    psgd_row_dp(ch, l0, h0, ln, ridx, rval, Pcol, k, act, deg, a);
                }
                if (o == 0 && c == 0)
                    list_continue<T, true>(lc, a, ac, ridx, rval, Pcol, k, deg, w, lin);
                else
                    list_continue<T, false>(lc, a, ac, ridx, rval, Pcol, k, deg, w, lin);
#pragma unroll
                for (int u = 0; u < kSampleNF; ++u)
                    if (act) part[u] += lams[s] * sample_top(ac[u], deg);
            }
        }
#pragma unroll
        for (int u = 0; u < kSampleNF; ++u) sc.put(i0 + u, group_sum(part[u], L) + lin[u], ln);
    }
    double ls;
    int fl = 0;
    list_coefs<L, EVAL>(sc, cf, M, list_loss, loss, ln, &ls, &fl);
    if (ln == 0) loss_row[at] = ls;
    if (EVAL) {
        if (ln == 0) first[at] = fl;
        return;
    }
    // passes 2 and 5 per (order, component chunk): the candidates again (cache-hot) into abar
    // with their own atomics, then one gradient pass over the context with abar
    for (int o = 0; o < n_orders; ++o) {
        const int deg = degree - o;
        for (int c = 0; c < C; ++c) {
            const int s = c * L + ln;
            const bool act = s < k;
            const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
            double* Gcol = grad_P + (size_t)o * d * k + (act ? s : 0);
            const double lam = act ? lams[s] : 0.0;
            if (!keep) {
                psgd_a_init(a);
                psgd_row_dp(ch, l0, h0, ln, ridx, rval, Pcol, k, act, deg, a);
            }
            double abar[kMaxDegree + 1];
#pragma unroll
            for (int t = 0; t <= kMaxDegree; ++t) abar[t] = 0.0;
            for (int i0 = 0; i0 <= M; i0 += kSampleNF) {
                lc.load(trow, i0, M, rptr);
                list_continue<T, false>(lc, a, ac, ridx, rval, Pcol, k, deg, w, nullptr);
                double cu[kSampleNF], cl[kSampleNF];
#pragma unroll
                for (int u = 0; u < kSampleNF; ++u) {
                    const double got = cf.get(i0 + u <= M ? i0 + u : M);  // (no shuffle in a branch)
                    cu[u] = (i0 + u <= M) ? got : 0.0;
                    cl[u] = cu[u] * lam;
#pragma unroll
                    for (int t = 1; t < kMaxDegree; ++t) abar[t] += cu[u] * ac[u][t];
                }
                list_cand_grad<T>(lc, ac, cl, cu, ridx, rval, Pcol, Gcol, k, deg, act,
                                  fit_linear && o == 0 && c == 0, ln, grad_w);
            }
            // abar[0] = sum_i coef_i is 0 by construction and is taken as exactly 0
            if (keep) {
                if (h0 > l0) ch.grad_from(abar, 0.0, deg, lam, Gcol, k, act);
                continue;
            }
            for (int64_t tb = l0; tb < h0; tb += kPsgdRC) {
                ch.load_entries(tb, h0, ln, ridx, rval);
                ch.load_p(Pcol, k, act);
                ch.grad_from(abar, 0.0, deg, lam, Gcol, k, act);
            }
        }
    }
}

// One L-lane group per list.  B lists from position pos0 of the visiting order (with a table:
// the batch of idx[0]); position r visits list q = list_order ? list_order[pos + r] : pos + r,
// the triples [qM, qM + M).  loss_row (and, EVAL, first) are indexed by position.
template <typename T, int L, bool EVAL>
__global__ __launch_bounds__(kBlock) void psgd_list_grad_kernel(
    const int32_t* __restrict__ triples, const int32_t* __restrict__ list_order, long long pos0,
    int B, int M, int list_loss, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const double* __restrict__ Pt,
    const double* __restrict__ w, const double* __restrict__ lams, int n_orders, int k, int d,
    int degree, int loss, int fit_linear, double* __restrict__ grad_P,
    double* __restrict__ grad_w, double* __restrict__ loss_row, int* __restrict__ first,
    const PsgdBatch* __restrict__ sched, int* __restrict__ idx) {
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    const int r = blockIdx.x * gpb + grp;
    if (sched) psgd_table_batch(sched, idx, B, pos0);
    if (r >= B) return;  // whole groups leave; no block-level synchronisation below
    const size_t at = (size_t)pos0 + (size_t)r;
    const size_t q = list_order ? (size_t)list_order[at] : at;
    const int32_t* trow = triples + 3 * q * (size_t)M;
    const int ib = trow[0];
    const int64_t l0 = rptr[ib], h0 = rptr[ib + 1];  // the context's entries
    if (n_orders == 1 && k <= L && h0 - l0 <= kPsgdRC)
        list_run<T, L, EVAL, true>(trow, at, l0, h0, M, list_loss, ln, rptr, ridx, rval, Pt, w,
                                   lams, n_orders, k, d, degree, loss, fit_linear, grad_P, grad_w,
                                   loss_row, first);
    else
        list_run<T, L, EVAL, false>(trow, at, l0, h0, M, list_loss, ln, rptr, ridx, rval, Pt, w,
                                    lams, n_orders, k, d, degree, loss, fit_linear, grad_P, grad_w,
                                    loss_row, first);
}

}  // namespace spfm
