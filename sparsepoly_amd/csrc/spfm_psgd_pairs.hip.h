// spfm_psgd_pairs.hip.h -- pairwise ranking gradient of the minibatch solver
// Part of the gfx950 device code of the sparse-FM solvers; see spfm_psgd.hip.h.
//
// A training example is a triple (b, c+, c-) of rows of the handle's one CSR image [X; Z]:
// context row b prefers candidate c+ to candidate c-.  With disjoint column sets the rows
// x_b + z_c are the concatenation of the two stored rows, so the ANOVA DP over x_b + z_c is the
// DP over the entries of b CONTINUED over the entries of c (a polynomial product: exact).
//   margin  m = f(x_b + z_c+) - f(x_b + z_c-)     (the context's linear term cancels)
//   loss      = loss_dev(loss, m, +1),  dL = dloss_dev(loss, m, +1)
//   grad_P[j] += dL lams_s (D+_j - D-_j)   j stored in b   (one atomic)
//              += +dL lams_s D+_j           j stored in c+
//              += -dL lams_s D-_j           j stored in c-
//   grad_w[j] += +dL z+_j / -dL z-_j       candidates' columns only
// where D+ / D- are the dprev recurrences of PsgdChunk::grad run with the DP arrays a+ / a- of
// the two summed rows.  An entry that is not part of a row enters that row's recurrences with
// x = 0: its DP update is a no-op and its D is 0, so no case distinction is left in the loops.
// What follows the gradient (psgd_update_kernel, the psgd_mich_* passes) is the pointwise
// solver's, unchanged.
//
// Weighted triples: the instances with WT read one double per triple,
// wt = weights[r] >= 0, write loss_row = wt * loss and scatter with dL = wt * dloss; a triple of
// weight 0 writes loss_row = 0 and leaves before any other load.  WT is a template parameter, not
// a null check at run time: the training instances fill the register file, and the instances
// without WT are the code of a build without weights.
#pragma once
#include "spfm_psgd.hip.h"

namespace spfm {

// The values of a chunk's entries as the two summed rows see them, spread over the lanes like
// PsgdChunk::xl: xp = x where the entry belongs to x_b + z_c+ (else 0), xm likewise for c-.
template <int L>
struct PairX {
    static constexpr int NT = kPsgdRC / L;
    double xp[NT], xm[NT];
    __device__ __forceinline__ double valp(int u) const { return __shfl(xp[u / L], u % L, L); }
    __device__ __forceinline__ double valm(int u) const { return __shfl(xm[u / L], u % L, L); }
    // a chunk of one row: the context (both), c+ (in_p alone) or c- (in_m alone)
    template <typename T>
    __device__ __forceinline__ void of_row(const PsgdChunk<T, L>& ch, bool in_p, bool in_m) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            xp[t] = in_p ? ch.xl[t] : 0.0;
            xm[t] = in_m ? ch.xl[t] : 0.0;
        }
    }
};

// The three rows of a triple packed into ONE chunk (together <= kPsgdRC entries): slots
// [0, nb) the context, [nb, nb + np) c+, [nb + np, nb + np + nm) c-.
template <typename T, int L>
__device__ __forceinline__ void pair_load_packed(PsgdChunk<T, L>& ch, PairX<L>& px, int64_t lob,
                                                 int nb, int64_t lop, int np, int64_t lom, int nm,
                                                 int ln, const int32_t* __restrict__ ridx,
                                                 const T* __restrict__ rval) {
    ch.cnt = nb + np + nm;
#pragma unroll
    for (int t = 0; t < PsgdChunk<T, L>::NT; ++t) {
        const int u = t * L + ln;
        const bool in = u < ch.cnt;
        const int64_t e = (u < nb) ? lob + u : (u < nb + np) ? lop + (u - nb) : lom + (u - nb - np);
        const double x = in ? (double)rval[e] : 0.0;  // 0 beyond the triple: every update a no-op
        ch.jl[t] = in ? ridx[e] : 0;
        ch.xl[t] = x;
        px.xp[t] = (u < nb + np) ? x : 0.0;
        px.xm[t] = (u < nb || u >= nb + np) ? x : 0.0;
    }
}

// DP of both summed rows over a packed chunk, continuing ap and am.  The context's recurrence
// is evaluated in both arrays -- the same values; what is shared is its loads, which are the
// cost.  DEG is the degree at compile time: gated by a run-time degree the 64 unrolled slots
// become one block of selects (the evaluation kernel then takes all 512 registers; with DEG
// it takes 256 + 59 and no scratch).
template <typename T, int L, int DEG>
__device__ __forceinline__ void pair_dp_packed(const PsgdChunk<T, L>& ch, const PairX<L>& px,
                                               double* ap, double* am) {
#pragma unroll
    for (int u = 0; u < kPsgdRC; ++u) {
        const double xp = px.valp(u), xm = px.valm(u);
#pragma unroll
        for (int t = DEG; t >= 1; --t) {
            ap[t] += ap[t - 1] * xp * ch.p[u];
            am[t] += am[t - 1] * xm * ch.p[u];
        }
    }
}

// Gradient scatter of a chunk: one atomic per entry of dl (D+ - D-), where D+ (D-) is 0 for an
// entry that is not part of x_b + z_c+ (x_b + z_c-).  DEG > 0: the degree at compile time
// (`deg` is not read).
template <typename T, int L, int DEG>
__device__ __forceinline__ void pair_grad(const PsgdChunk<T, L>& ch, const PairX<L>& px,
                                          const double* ap, const double* am, int deg, double dl,
                                          double* __restrict__ Gcol, int k, bool act) {
    if (DEG) deg = DEG;
#pragma unroll
    for (int u = 0; u < kPsgdRC; ++u) {
        const int j = ch.col(u);
        const double xp = px.valp(u), xm = px.valm(u);
        double dp = xp, dm = xm;
#pragma unroll
        for (int t = 1; t < kMaxDegree; ++t)
            if (t < deg) {
                dp = xp * (ap[t] - ch.p[u] * dp);
                dm = xm * (am[t] - ch.p[u] * dm);
            }
        if (act && u < ch.cnt) unsafeAtomicAdd(&Gcol[(size_t)j * k], dl * (dp - dm));
    }
}

// DP arrays of the two summed rows of one (order, component chunk) in the chunked form: the
// context's DP once, copied, then continued over c+ (-> ap) and over c- (-> am).  [l0, h0),
// [l1, h1), [l2, h2): the entries of the context, c+ and c-.  Every trip count is uniform within
// the group.
template <typename T, int L>
__device__ __forceinline__ void pair_dp_rows(PsgdChunk<T, L>& ch, int64_t l0, int64_t h0,
                                             int64_t l1, int64_t h1, int64_t l2, int64_t h2,
                                             int ln, const int32_t* __restrict__ ridx,
                                             const T* __restrict__ rval,
                                             const double* __restrict__ Pcol, int k, bool act,
                                             int deg, double* ap, double* am) {
    psgd_a_init(ap);
    psgd_row_dp(ch, l0, h0, ln, ridx, rval, Pcol, k, act, deg, ap);
#pragma unroll
    for (int t = 0; t <= kMaxDegree; ++t) am[t] = ap[t];
    psgd_row_dp(ch, l1, h1, ln, ridx, rval, Pcol, k, act, deg, ap);
    psgd_row_dp(ch, l2, h2, ln, ridx, rval, Pcol, k, act, deg, am);
}

// a+[deg] - a-[deg].  Every order's difference is formed first and the one wanted is selected
// among VALUES: a selection among the array elements themselves becomes an indexed load, which
// moves both arrays out of the registers.  (One of three forms of this selection, each fitted to
// its kernel's registers: sample_top in spfm_psgd_sample.hip.h sums masked values, psgd_grad_kernel
// selects inline among the values of its one array.)
__device__ __forceinline__ double pair_top_diff(const double* ap, const double* am, int deg) {
    double df[kMaxDegree + 1];
#pragma unroll
    for (int t = 1; t <= kMaxDegree; ++t) df[t] = ap[t] - am[t];
    double top = df[1];
#pragma unroll
    for (int t = 2; t <= kMaxDegree; ++t)
        if (t == deg) top = df[t];
    return top;
}

// The margin's way out, shared by both forms of the kernel: reduce it over the group, write the
// triple's loss (EVAL: and the 0/1 flag m > 0), scatter the candidates' part of grad_w (no
// atomic ever touches a context column).  Returns dL.  WT: loss and dL times weights[r], read
// here and not carried through the DP.
template <typename T, int L, bool EVAL, bool WT>
__device__ __forceinline__ double pair_margin_out(double m, int64_t l1, int64_t h1, int64_t l2,
                                                  int64_t h2, int ln, int r, int loss,
                                                  int fit_linear, const int32_t* __restrict__ ridx,
                                                  const T* __restrict__ rval,
                                                  double* __restrict__ grad_w,
                                                  double* __restrict__ loss_row,
                                                  int* __restrict__ ordered,
                                                  const double* __restrict__ weights) {
    m = group_sum(m, L);
    if (WT) {
        if (ln == 0) loss_row[r] = weights[r] * loss_dev(loss, m, 1.0);
    } else {
        if (ln == 0) loss_row[r] = loss_dev(loss, m, 1.0);
    }
    if (EVAL) {
        if (ln == 0) ordered[r] = m > 0.0 ? 1 : 0;
        return 0.0;
    }
    const double dL = WT ? weights[r] * dloss_dev(loss, m, 1.0) : dloss_dev(loss, m, 1.0);
    if (fit_linear) {
        for (int64_t e = l1 + ln; e < h1; e += L)
            unsafeAtomicAdd(&grad_w[ridx[e]], dL * (double)rval[e]);
        for (int64_t e = l2 + ln; e < h2; e += L)
            unsafeAtomicAdd(&grad_w[ridx[e]], -dL * (double)rval[e]);
    }
    return dL;
}

// The register-resident form of one triple at degree DEG: the packed chunk -- entries and P
// values -- stays in registers between the margin and the gradient.
template <typename T, int L, bool EVAL, int DEG, bool WT>
__device__ __forceinline__ void pair_keep(int64_t l0, int nb, int64_t l1, int np, int64_t l2,
                                          int nm, double m, int ln, int r, int k, int loss,
                                          int fit_linear, const int32_t* __restrict__ ridx,
                                          const T* __restrict__ rval,
                                          const double* __restrict__ Pt,
                                          const double* __restrict__ lams,
                                          double* __restrict__ grad_P, double* __restrict__ grad_w,
                                          double* __restrict__ loss_row,
                                          int* __restrict__ ordered,
                                          const double* __restrict__ weights) {
    const bool act = ln < k;
    PsgdChunk<T, L> ch;
    PairX<L> px;
    double ap[kMaxDegree + 1], am[kMaxDegree + 1];
    pair_load_packed(ch, px, l0, nb, l1, np, l2, nm, ln, ridx, rval);
    ch.load_p(Pt + (act ? ln : 0), k, act);
    psgd_a_init(ap);
    psgd_a_init(am);
    pair_dp_packed<T, L, DEG>(ch, px, ap, am);
    if (act) m += lams[ln] * (ap[DEG] - am[DEG]);
    const double dL = pair_margin_out<T, L, EVAL, WT>(m, l1, l1 + np, l2, l2 + nm, ln, r, loss,
                                                      fit_linear, ridx, rval, grad_w, loss_row,
                                                      ordered, weights);
    if (EVAL) return;
    pair_grad<T, L, DEG>(ch, px, ap, am, DEG, act ? dL * lams[ln] : 0.0, grad_P + (act ? ln : 0),
                         k, act);
}

// One L-lane group per triple.  EVAL: no gradient; loss_row[r] and ordered[r] = (m > 0).
// WT: `weights` holds one double per slot of `triples` (else it is not read).
template <typename T, int L, bool EVAL, bool WT = false>
__global__ __launch_bounds__(kBlock) void psgd_pair_grad_kernel(
    const int32_t* __restrict__ triples, int B, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const double* __restrict__ Pt,
    const double* __restrict__ w, const double* __restrict__ lams, int n_orders, int k, int d,
    int degree, int loss, int fit_linear, double* __restrict__ grad_P,
    double* __restrict__ grad_w, double* __restrict__ loss_row, int* __restrict__ ordered,
    const PsgdBatch* __restrict__ sched, int* __restrict__ idx,
    const double* __restrict__ weights) {
    static_assert(!(EVAL && WT), "the evaluation is unweighted");
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    const int r = blockIdx.x * gpb + grp;
    if (sched) {
        long long pos;
        psgd_table_batch(sched, idx, B, pos);
        triples += 3 * pos;
        loss_row += pos;
        if (WT) weights += pos;
    }
    if (r >= B) return;  // whole groups leave; no block-level synchronisation below
    if (WT) {
        if (weights[r] == 0.0) {  // the same r in all lanes of the group: it leaves as a whole
            if (ln == 0) loss_row[r] = 0.0;
            return;
        }
    }
    const int ib = triples[3 * (size_t)r], ip = triples[3 * (size_t)r + 1],
              im = triples[3 * (size_t)r + 2];
    const int64_t l0 = rptr[ib], h0 = rptr[ib + 1];  // the context's entries
    const int64_t l1 = rptr[ip], h1 = rptr[ip + 1];  // c+
    const int64_t l2 = rptr[im], h2 = rptr[im + 1];  // c-
    const int C = (k + L - 1) / L;
    // the candidates' linear terms; the context's cancels in the margin and is never formed
    double m = 0.0;
    for (int64_t e = l1 + ln; e < h1; e += L) m += (double)rval[e] * w[ridx[e]];
    for (int64_t e = l2 + ln; e < h2; e += L) m -= (double)rval[e] * w[ridx[e]];
    // the common shape (one order, k <= L, the THREE rows fit one chunk together) keeps the
    // packed chunk in registers (pair_keep, one instance per degree); the two forms share no
    // state and each runs to its own end
    if (n_orders == 1 && C == 1 && (h0 - l0) + (h1 - l1) + (h2 - l2) <= kPsgdRC) {
#define SPFM_PAIR_KEEP(DEG)                                                                    \
    case DEG:                                                                                  \
        pair_keep<T, L, EVAL, DEG, WT>(l0, (int)(h0 - l0), l1, (int)(h1 - l1), l2,             \
                                       (int)(h2 - l2), m, ln, r, k, loss, fit_linear, ridx,    \
                                       rval, Pt, lams, grad_P, grad_w, loss_row, ordered,      \
                                       weights);                                               \
        break
        switch (degree) {
            SPFM_PAIR_KEEP(2);
            SPFM_PAIR_KEEP(3);
            SPFM_PAIR_KEEP(4);
            SPFM_PAIR_KEEP(5);
            SPFM_PAIR_KEEP(6);
        }
#undef SPFM_PAIR_KEEP
        return;
    }
    PsgdChunk<T, L> ch;
    double ap[kMaxDegree + 1], am[kMaxDegree + 1];
    for (int o = 0; o < n_orders; ++o) {
        const int deg = degree - o;
        for (int c = 0; c < C; ++c) {
            const int s = c * L + ln;
            const bool act = s < k;
            pair_dp_rows(ch, l0, h0, l1, h1, l2, h2, ln, ridx, rval,
                         Pt + (size_t)o * d * k + (act ? s : 0), k, act, deg, ap, am);
            if (act) m += lams[s] * pair_top_diff(ap, am, deg);
        }
    }
    const double dL = pair_margin_out<T, L, EVAL, WT>(m, l1, h1, l2, h2, ln, r, loss, fit_linear,
                                                      ridx, rval, grad_w, loss_row, ordered,
                                                      weights);
    if (EVAL) return;
    PairX<L> px;
    for (int o = 0; o < n_orders; ++o) {
        const int deg = degree - o;
        for (int c = 0; c < C; ++c) {
            const int s = c * L + ln;
            const bool act = s < k;
            const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
            double* Gcol = grad_P + (size_t)o * d * k + (act ? s : 0);
            const double dl = act ? dL * lams[s] : 0.0;
            pair_dp_rows(ch, l0, h0, l1, h1, l2, h2, ln, ridx, rval, Pcol, k, act, deg, ap, am);
            for (int q = 0; q < 3; ++q) {  // the context: both rows; c+: a+ alone; c-: a- alone
                const int64_t lq = q == 0 ? l0 : q == 1 ? l1 : l2;
                const int64_t hq = q == 0 ? h0 : q == 1 ? h1 : h2;
                for (int64_t tb = lq; tb < hq; tb += kPsgdRC) {
                    ch.load_entries(tb, hq, ln, ridx, rval);
                    ch.load_p(Pcol, k, act);
                    px.of_row(ch, q != 2, q != 1);
                    pair_grad<T, L, 0>(ch, px, ap, am, deg, dl, Gcol, k, act);
                }
            }
        }
    }
}

}  // namespace spfm
