// spfm_psgd_sample.hip.h -- negatives of the pairwise fit, drawn on the device
// Part of the gfx950 device code of the sparse-FM solvers; see spfm_psgd_pairs.hip.h.
//
// Output triple r = q * n_negatives + i is the i-th negative of positive q (context b, candidate
// c+; positives in the canonical CSR order of `interactions`).  Its draws are
//   u_t = draw_u64(seed, epoch, r, t),  t = 0, 1, ...      candidate ((u_t >> 32) * C) >> 32
// and a draw is admitted when its candidate is not stored in row b of the forbidden CSR
// (interactions and exclude together, sorted).  The candidate set of r is the first M admitted
// draws among t < max_draws (repeats allowed; fewer than M: those; none: the first admissible
// candidate on the cyclic walk upwards from the last drawn one).  The chosen negative is the
// candidate of the set with the largest score
//   s(b, c) = sum_o sum_s lams_s a_s^{degree-o}(x_b + z_c) + <w, z_c>
// (the context's linear term is the same for all of them and is left out), ties to the earliest
// admitted draw.  M == 1 scores nothing: the uniform sampler.
//
// DESIGN.md section 19c adds three things, each off by default with today's output bit for bit:
//  * a proposal table `cum` (inclusive cumulative sums of integer weights, W = cum[C - 1]): the
//    candidate of a draw is the smallest c with cum[c] > ((u >> 32) * W) >> 32 -- the same
//    multiply-shift, then a binary search; admission and the fallback walk do not change (the
//    walk may therefore end on a candidate of weight 0);
//  * WARP (the template parameter): the positive is scored first, the admitted draws are tried in
//    the order of t and the first whose score exceeds s+ - margin (the violator, trial N) is the
//    negative, with weight posw_q log(max(1, floor(A_b / N))), A_b = C - |forbidden(b)|; if none
//    of the (at most M) tried violates: the highest-scored of them, weight 0, trials 0;
//  * positive weights posw (one per positive, canonical order): the plain modes write
//    weights[slot] = posw_q, WARP the product above.
#pragma once
#include "spfm_psgd.hip.h"

namespace spfm {

constexpr int kSampleNF = 4;  // candidates of one context scored side by side

__host__ __device__ __forceinline__ uint64_t sample_mix64(uint64_t z) {  // splitmix64 finaliser
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// The stream key of triple r in (seed, epoch); draw t of the stream is the splitmix64 output
// t + 1 from that state.  Integer arithmetic modulo 2^64 only (pairwise.draw_u64 restates it).
__host__ __device__ __forceinline__ uint64_t sample_key(uint64_t seed, uint64_t epoch, uint64_t r) {
    const uint64_t a = sample_mix64((seed << 32) ^ (epoch & 0xFFFFFFFFull));
    return sample_mix64(a ^ (r * 0x9E3779B97F4A7C15ull));
}
__host__ __device__ __forceinline__ uint64_t sample_draw(uint64_t key, uint64_t t) {
    return sample_mix64(key + (t + 1) * 0x9E3779B97F4A7C15ull);
}
// cum == nullptr: uniform over [0, C); else the table's draw (cum[C - 1] = W > x: it ends inside)
__device__ __forceinline__ int sample_cand(uint64_t u, int C, const uint32_t* __restrict__ cum,
                                           uint32_t W) {
    if (!cum) return (int)(((u >> 32) * (uint64_t)C) >> 32);
    const uint32_t x = (uint32_t)(((u >> 32) * (uint64_t)W) >> 32);
    int lo = 0, hi = C - 1;  // the smallest c with cum[c] > x
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > x)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// is c stored in the sorted list idx[lo, hi)?
__device__ __forceinline__ bool sample_stored(const int32_t* __restrict__ idx, int64_t lo,
                                              int64_t hi, int c) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int v = idx[mid];
        if (v == c) return true;
        if (v < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    return false;
}

// a[deg] as a sum of masked values (exact: one term, the rest zeros).  A selection among the
// array elements themselves becomes an indexed load and moves the DP arrays of the candidates in
// flight to scratch (240 bytes per lane in every instance; see pair_top_diff).  (The other two
// forms of this selection: pair_top_diff in spfm_psgd_pairs.hip.h, and the inline one of
// psgd_grad_kernel in spfm_psgd.hip.h.)
__device__ __forceinline__ double sample_top(const double* a, int deg) {
    double top = 0.0;
#pragma unroll
    for (int t = 1; t <= kMaxDegree; ++t) top += (t == deg) ? a[t] : 0.0;
    return top;
}

// s(b, c) of ONE candidate row [lc, lc + nc) for the whole group (the fallback candidate, the
// positive of WARP): the DP of the context (`a` when kept, else formed per order and component
// chunk) continued over the candidate's entries.  Uniform trip counts.
template <typename T, int L>
__device__ __forceinline__ double sample_score_one(
    int64_t lc, int nc, int64_t l0, int64_t h0, bool keep, double* a, int ln,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const double* __restrict__ Pt,
    const double* __restrict__ w, const double* __restrict__ lams, int n_orders, int NC, int k,
    int d, int degree) {
    double part = 0.0, lin = 0.0;
    for (int o = 0; o < n_orders; ++o) {
        const int deg = degree - o;
        for (int cc = 0; cc < NC; ++cc) {
            const int s = cc * L + ln;
            const bool act = s < k;
            const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
            if (!keep) {
                PsgdChunk<T, L> ch;
                psgd_a_init(a);
                psgd_row_dp(ch, l0, h0, ln, ridx, rval, Pcol, k, act, deg, a);
            }
            double ac[kMaxDegree + 1];
#pragma unroll
            for (int tt = 0; tt <= kMaxDegree; ++tt) ac[tt] = a[tt];
            for (int e = 0; e < nc; ++e) {
                const int j = ridx[lc + e];
                const double x = (double)rval[lc + e];
                const double p = Pcol[(size_t)j * k];
                if (o == 0 && cc == 0) lin += x * w[j];
#pragma unroll
                for (int tt = kMaxDegree; tt >= 1; --tt)
                    if (tt <= deg) ac[tt] += ac[tt - 1] * x * p;
            }
            if (act) part += lams[s] * sample_top(ac, deg);
        }
    }
    return group_sum(part, L) + lin;
}

// One L-lane group per output triple.  Every loop below that holds a group shuffle or a ballot
// has a trip count that is uniform within the group: the draws, the admitted mask, the counts
// and the candidates' rows are the same in all of its lanes -- and so are the scores, so WARP's
// exit at the first violator is taken by the group as a whole.  WARP: M is the number of trials;
// candidates that share a batch of kSampleNF with the violator and come after it are scored and
// ignored.  cum / posw / weights / trials may be null (trials: WARP only).
template <typename T, int L, bool WARP = false>
__global__ __launch_bounds__(kBlock) void psgd_pair_sample_kernel(
    int m, int n_neg, int M, int max_draws, uint64_t seed, uint64_t epoch, int n_ctx, int C,
    const int32_t* __restrict__ pos_row, const int32_t* __restrict__ pos_idx,
    const int64_t* __restrict__ fptr, const int32_t* __restrict__ fidx,
    const int32_t* __restrict__ order, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const double* __restrict__ Pt,
    const double* __restrict__ w, const double* __restrict__ lams, int n_orders, int k, int d,
    int degree, int32_t* __restrict__ triples, double* __restrict__ scores,
    const uint32_t* __restrict__ cum, uint32_t W, const double* __restrict__ posw, double margin,
    double* __restrict__ weights, int32_t* __restrict__ trials) {
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    const int r = blockIdx.x * gpb + grp;
    if (r >= m) return;  // whole groups leave; no block-level synchronisation below
    const int q = r / n_neg;
    const int b = pos_row[q], cplus = pos_idx[q];
    const int64_t f0 = fptr[b], f1 = fptr[b + 1];
    const uint64_t key = sample_key(seed, epoch, (uint64_t)r);
    const int gbase = (threadIdx.x & 63) - ln;  // the group's first lane within its wave
    const uint64_t gmask = (L >= 64) ? ~0ull : ((1ull << (L & 63)) - 1);

    const int64_t l0 = rptr[b], h0 = rptr[b + 1];  // the context's entries
    const int NC = (k + L - 1) / L;
    // the context's DP is formed once and every candidate continues a copy of it: one order,
    // k <= L and a context of one chunk (else: per candidate batch, order and component chunk)
    const bool keep = (n_orders == 1 && NC == 1 && h0 - l0 <= kPsgdRC);
    double a[kMaxDegree + 1];
    if ((WARP || M > 1) && keep) {
        PsgdChunk<T, L> ch;
        const bool act = ln < k;
        psgd_a_init(a);
        psgd_row_dp(ch, l0, h0, ln, ridx, rval, Pt + (act ? ln : 0), k, act, degree, a);
    }

    // WARP: the violation threshold s+ - margin and the trial that crossed it (0: none yet)
    double thr = 0.0;
    int found = 0;
    if (WARP) {
        const int64_t lp = rptr[n_ctx + cplus];
        thr = sample_score_one<T, L>(lp, (int)(rptr[n_ctx + cplus + 1] - lp), l0, h0, keep, a, ln,
                                     ridx, rval, Pt, w, lams, n_orders, NC, k, d, degree) -
              margin;
    }

    int best = -1, cnt = 0;
    double best_s = 0.0;
    for (int64_t t0 = 0; t0 < max_draws && cnt < M && !found; t0 += L) {
        const int64_t t = t0 + ln;
        const int mine = sample_cand(sample_draw(key, (uint64_t)t), C, cum, W);
        const bool adm = t < max_draws && !sample_stored(fidx, f0, f1, mine);
        uint64_t mask = (__ballot(adm) >> gbase) & gmask;  // admitted draws of this round, by t
        if (!WARP && M == 1) {
            if (mask) {
                best = __shfl(mine, __ffsll((unsigned long long)mask) - 1, L);
                cnt = 1;
            }
            continue;
        }
        while (mask && cnt < M && !found) {
            // the next (up to) kSampleNF admitted candidates, in the order of their draws
            int cand[kSampleNF], len[kSampleNF];
            int64_t lo[kSampleNF];
            int nb = 0, maxlen = 0;
#pragma unroll
            for (int u = 0; u < kSampleNF; ++u) {
                const bool on = mask != 0 && cnt + u < M;
                const int src = on ? __ffsll((unsigned long long)mask) - 1 : 0;
                const int c = __shfl(mine, src, L);
                cand[u] = on ? c : -1;
                lo[u] = on ? rptr[n_ctx + c] : 0;
                len[u] = on ? (int)(rptr[n_ctx + c + 1] - lo[u]) : 0;
                maxlen = len[u] > maxlen ? len[u] : maxlen;
                if (on) {
                    mask &= mask - 1;
                    nb += 1;
                }
            }
            double part[kSampleNF], lin[kSampleNF];
#pragma unroll
            for (int u = 0; u < kSampleNF; ++u) part[u] = lin[u] = 0.0;
            for (int o = 0; o < n_orders; ++o) {
                const int deg = degree - o;
                for (int c = 0; c < NC; ++c) {
                    const int s = c * L + ln;
                    const bool act = s < k;
                    const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
                    if (!keep) {
                        PsgdChunk<T, L> ch;
                        psgd_a_init(a);
                        psgd_row_dp(ch, l0, h0, ln, ridx, rval, Pcol, k, act, deg, a);
                    }
                    double ac[kSampleNF][kMaxDegree + 1];
#pragma unroll
                    for (int u = 0; u < kSampleNF; ++u)
#pragma unroll
                        for (int tt = 0; tt <= kMaxDegree; ++tt) ac[u][tt] = a[tt];
                    // rolled over the candidates' own (short) rows; every lane reads the same
                    // entry, so no shuffle is needed and the loads of the batch overlap
                    for (int e = 0; e < maxlen; ++e) {
#pragma unroll
                        for (int u = 0; u < kSampleNF; ++u) {
                            const bool in = e < len[u];
                            const int64_t pe = lo[u] + (in ? e : 0);
                            const int j = in ? ridx[pe] : 0;
                            const double x = in ? (double)rval[pe] : 0.0;
                            const double p = Pcol[(size_t)j * k];
                            if (o == 0 && c == 0) lin[u] += x * w[j];
#pragma unroll
                            for (int tt = kMaxDegree; tt >= 1; --tt)
                                if (tt <= deg) ac[u][tt] += ac[u][tt - 1] * x * p;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kSampleNF; ++u)
                        if (act) part[u] += lams[s] * sample_top(ac[u], deg);
                }
            }
#pragma unroll
            for (int u = 0; u < kSampleNF; ++u) {
                const double sc = group_sum(part[u], L) + lin[u];
                if (WARP) {
                    if (u < nb && !found) {
                        if (sc > thr) {  // the violator: what was tried before it is dropped
                            found = cnt + u + 1;
                            best = cand[u];
                            best_s = sc;
                        } else if (best < 0 || sc > best_s) {
                            best = cand[u];
                            best_s = sc;
                        }
                    }
                } else if (u < nb && (best < 0 || sc > best_s)) {  // ties: the earliest admitted draw
                    best = cand[u];
                    best_s = sc;
                }
            }
            cnt += nb;
        }
    }
    if (best < 0) {  // no draw admitted: walk upwards from the last drawn candidate
        int c = sample_cand(sample_draw(key, (uint64_t)(max_draws - 1)), C, cum, W);
        for (int step = 0; step < C; ++step) {
            c = (c + 1 == C) ? 0 : c + 1;
            if (!sample_stored(fidx, f0, f1, c)) break;
        }
        best = c;  // (the set-up check guarantees an admissible candidate)
        // its score, for the score buffer (M == 1 without WARP: not formed)
        if (WARP || M > 1) {
            const int64_t lc = rptr[n_ctx + c];
            best_s = sample_score_one<T, L>(lc, (int)(rptr[n_ctx + c + 1] - lc), l0, h0, keep, a,
                                            ln, ridx, rval, Pt, w, lams, n_orders, NC, k, d,
                                            degree);
        }
    }
    if (ln == 0) {
        const size_t slot = order ? (size_t)order[r] : (size_t)r;
        triples[3 * slot] = b;
        triples[3 * slot + 1] = n_ctx + cplus;
        triples[3 * slot + 2] = n_ctx + best;
        scores[slot] = best_s;
        if (weights) {
            double wt = posw ? posw[q] : 1.0;
            if (WARP) {
                const int64_t rank = found ? ((int64_t)C - (f1 - f0)) / found : 0;
                wt = rank > 1 ? wt * log((double)rank) : 0.0;
            }
            weights[slot] = wt;
        }
        if (WARP && trials) trials[slot] = found;
    }
}

}  // namespace spfm
