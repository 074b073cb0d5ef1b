// spfm_psgd_det.hip.h -- the deterministic minibatch gradient of psgd
// Part of the gfx950 device code of the sparse-FM solvers; see spfm_kernels.hip.h.
//
// psgd_grad_kernel (spfm_psgd.hip.h) scatters a row's terms with f64 atomics, so a column's sum is
// taken in the order the hardware delivers them.  Here the same terms are added in a fixed order:
//   grad_P[o, j, s] = sum over the rows r of the minibatch that store column j, r ascending, of
//                     (dL_r lams_s) * d a_s^deg(x_r) / d p_sj          grad_w[j] likewise of dL_r x_rj
// which is the order of the reference's _update_grads (psgd.py:60-91).  Per epoch a plan sorts the
// stored entries by (minibatch, column) -- stable, so r ascends inside a segment -- and per
// minibatch two kernels run:
//   psgd_rowstate_kernel  the front half of psgd_grad_kernel (one L-lane group per row): DP,
//                         prediction, dL_r, loss_row; it stores dL_r and the row's DP values
//                         a_s^1 .. a_s^{deg-1} per order (a_s^0 = 1 is not stored) and writes no
//                         gradient
//   psgd_colgrad_kernel   one L-lane group per segment (lane = component): per entry it rebuilds
//                         d a / d p by psgd_grad_kernel's downward recurrence from the row's stored
//                         a and adds the term into a register; one plain store per (o, j, s)
// A segment longer than kDetSeg entries is cut into pieces of kDetSeg; piece partials start from
// zero and are added in ascending piece order, so the shape of the sum is a function of the
// segment's length alone.  The pieces of a long segment stay in one workgroup: its kBlock / L
// groups take a piece each and group 0 folds the partials through LDS in piece order -- no
// scratch in memory, no second launch, and nothing in the recorded graph depends on the data.
// No float atomics anywhere; update and Michelot kernels are those of spfm_psgd.hip.h.
#pragma once
#include "spfm_psgd.hip.h"

namespace spfm {

constexpr int kDetSeg = 256;  // entries of a piece
constexpr int kDetU = 16;     // entries whose state loads are in flight together

// The epoch's plan as the gradient kernels see it: the entries of minibatch b's segments
// [bseg_ptr[b], bseg_ptr[b + 1]) sorted by column, segment s holding the records
// [seg_ptr[s], seg_ptr[s + 1]) of column seg_col[s]; record = (row's position in its minibatch,
// value in rec_x of the storage type).
struct DetPlan {
    const int32_t* bseg_ptr;
    const int32_t* seg_ptr;
    const int32_t* seg_col;
    const int32_t* rec_r;
};

// ------------------------------------------------------------------ the plan's kernels
// len[q] = stored entries of the row visited at position q
static __global__ __launch_bounds__(kBlock) void det_rowlen_kernel(
    const int32_t* __restrict__ samples, const int64_t* __restrict__ rptr, int64_t n,
    int64_t* __restrict__ len) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n) return;
    const int i = samples[q];
    len[q] = rptr[i + 1] - rptr[i];
}

// one record per stored entry, in position order (16 lanes per position): entry m = qoff[q] + t of
// the stream gets key (q / batch_size) * d + column, value m, and ent_q[m] = q
static __global__ __launch_bounds__(kBlock) void det_enum_kernel(
    const int32_t* __restrict__ samples, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const int64_t* __restrict__ qoff, int64_t n,
    int64_t batch_size, int d, uint64_t* __restrict__ key, uint32_t* __restrict__ val,
    int32_t* __restrict__ ent_q) {
    const int64_t q = (int64_t)blockIdx.x * (kBlock / 16) + threadIdx.x / 16;
    if (q >= n) return;
    const int i = samples[q];
    const int64_t lo = rptr[i], len = rptr[i + 1] - lo, base = qoff[q];
    const uint64_t kb = (uint64_t)(q / batch_size) * (uint64_t)d;
    for (int64_t t = threadIdx.x % 16; t < len; t += 16) {
        key[base + t] = kb + (uint64_t)ridx[lo + t];
        val[base + t] = (uint32_t)(base + t);
        ent_q[base + t] = (int32_t)q;
    }
}

// behind the sort: the records in sorted order and the head flag of every (minibatch, column) run
template <typename T>
__global__ __launch_bounds__(kBlock) void det_head_kernel(
    const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
    const int32_t* __restrict__ ent_q, const int32_t* __restrict__ samples,
    const int64_t* __restrict__ rptr, const T* __restrict__ rval,
    const int64_t* __restrict__ qoff, int64_t N, int64_t batch_size, int32_t* __restrict__ rec_r,
    T* __restrict__ rec_x, int32_t* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= N) return;
    const int64_t m = val[t];
    const int64_t q = ent_q[m];
    rec_r[t] = (int32_t)(q % batch_size);
    rec_x[t] = rval[rptr[samples[q]] + (m - qoff[q])];
    flag[t] = (t == 0 || key[t] != key[t - 1]) ? 1 : 0;
}

// sid1 = inclusive scan of the head flags.  Every head writes its segment; the first head of a
// minibatch also writes bseg_ptr of that minibatch and of the entry-less ones before it; the last
// record closes the tables.  figs[0] = number of segments.
static __global__ __launch_bounds__(kBlock) void det_seg_kernel(
    const uint64_t* __restrict__ key, const int32_t* __restrict__ flag,
    const int32_t* __restrict__ sid1, int64_t N, int d, int64_t nbat, int32_t* __restrict__ seg_ptr,
    int32_t* __restrict__ seg_col, int32_t* __restrict__ bseg_ptr, int* __restrict__ figs) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= N) return;
    const int64_t b = (int64_t)(key[t] / (uint64_t)d);
    if (flag[t]) {
        const int s = sid1[t] - 1;
        seg_ptr[s] = (int32_t)t;
        seg_col[s] = (int32_t)(key[t] % (uint64_t)d);
        const int64_t pb = t == 0 ? -1 : (int64_t)(key[t - 1] / (uint64_t)d);
        for (int64_t bb = pb + 1; bb <= b; ++bb) bseg_ptr[bb] = s;
    }
    if (t == N - 1) {
        const int nseg = sid1[t];
        seg_ptr[nseg] = (int32_t)N;
        for (int64_t bb = b + 1; bb <= nbat; ++bb) bseg_ptr[bb] = nseg;
        figs[0] = nseg;
    }
}

// figs[1] = entries of the longest segment (integer max: no order to fix)
static __global__ __launch_bounds__(kBlock) void det_longest_kernel(
    const int32_t* __restrict__ seg_ptr, int64_t N, int* __restrict__ figs) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int len = 0;
    if (s < N && s < figs[0]) len = seg_ptr[s + 1] - seg_ptr[s];
    for (int m = kWave >> 1; m >= 1; m >>= 1) len = max(len, __shfl_xor(len, m, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0 && len > 0) atomicMax(&figs[1], len);
}

// flag[0] = 1 if the two orders differ (the caller cleared it)
static __global__ __launch_bounds__(kBlock) void det_differ_kernel(
    const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t n,
    int* __restrict__ flag) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q < n && a[q] != b[q]) flag[0] = 1;  // (every writer stores the same 1)
}

// ------------------------------------------------------------------ the gradient kernels
// The front half of psgd_grad_kernel for the rows of one minibatch, on a fixed grid (the rows are
// walked with a grid stride): dLrow[r], loss_row[r], and the DP values of row r in
//   state[((r * n_orders + o) * (degree - 1) + (t - 1)) * k + s] = a_s^t,  t = 1 .. degree - o - 1
// (k contiguous: one coalesced line per (row, order, t)).  No gradient is written.
template <typename T, int L, typename WA = NoRowWeight>
__global__ __launch_bounds__(kBlock) void psgd_rowstate_kernel(
    const int32_t* __restrict__ samples, int B, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const T* __restrict__ yy,
    const double* __restrict__ Pt, const double* __restrict__ w,
    const double* __restrict__ lams, int n_orders, int k, int d, int degree, int loss,
    double* __restrict__ dLrow, double* __restrict__ state, double* __restrict__ loss_row,
    const PsgdBatch* __restrict__ sched, int* __restrict__ idx, WA wt) {
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    if (sched) {
        long long pos;
        psgd_table_batch(sched, idx, B, pos);
        samples += pos;
        loss_row += pos;
    }
    const int C = (k + L - 1) / L;
    const int nst = degree - 1;
    PsgdChunk<T, L> ch;
    double a[kMaxDegree + 1];
    for (int r = blockIdx.x * gpb + grp; r < B; r += gridDim.x * gpb) {  // whole groups
        const int i = samples[r];
        const int64_t lo = rptr[i], hi = rptr[i + 1];
        const double yi = (double)yy[2 * (size_t)i + 1];
        // _pred (psgd.py:47-57), the expressions of psgd_grad_kernel
        double yp = 0.0;
        for (int64_t e = lo + ln; e < hi; e += L) yp += (double)rval[e] * w[ridx[e]];
        for (int o = 0; o < n_orders; ++o) {
            const int deg = degree - o;
            for (int c = 0; c < C; ++c) {
                const int s = c * L + ln;
                const bool act = s < k;
                const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
                psgd_a_init(a);
                psgd_row_dp(ch, lo, hi, ln, ridx, rval, Pcol, k, act, deg, a);
                double top = a[1];
#pragma unroll
                for (int t = 2; t <= kMaxDegree; ++t)
                    if (t == deg) top = a[t];
                if (act) {
                    yp += lams[s] * top;
                    double* st = state + (((size_t)r * n_orders + o) * nst) * k + s;
#pragma unroll
                    for (int t = 1; t < kMaxDegree; ++t)
                        if (t < deg) st[(size_t)(t - 1) * k] = a[t];
                }
            }
        }
        yp = group_sum(yp, L);
        double dL, ls;
        if constexpr (WA::on) {
            const double wi = wt((size_t)i);
            dL = wi * dloss_dev(loss, yp, yi);
            ls = wi * loss_dev(loss, yp, yi);
        } else {
            dL = dloss_dev(loss, yp, yi);
            ls = loss_dev(loss, yp, yi);
        }
        if (ln == 0) {
            loss_row[r] = ls;
            dLrow[r] = dL;
        }
    }
}

// The partial sums of the records [e0, e1) (one piece, <= kDetSeg) for one component lane of one
// order, in record order from zero: gp of (dL lam) * d a^deg / d p, gw of dL x.  The records are
// loaded L at a time, lane-parallel, and broadcast with group shuffles as PsgdChunk does, so the
// dependent state loads of kDetU entries are issued back to back.  `st`: the state of row 0 for
// this (order, lane); term and recurrence are PsgdChunk::grad's.
template <typename T, int L>
__device__ __forceinline__ void det_piece(int e0, int e1, int ln, const int32_t* __restrict__ rec_r,
                                          const T* __restrict__ rec_x,
                                          const double* __restrict__ dLrow,
                                          const double* __restrict__ st, size_t rstride, int k,
                                          int deg, double lam, double p, bool act, double& gp,
                                          double& gw) {
    gp = 0.0;
    gw = 0.0;
    for (int tb = e0; tb < e1; tb += L) {
        const int e = tb + ln;
        const bool in = e < e1;
        const int rl = in ? rec_r[e] : 0;
        const double xl = in ? (double)rec_x[e] : 0.0;
        const double dl = in ? dLrow[rl] : 0.0;
        const int cnt = (e1 - tb < L) ? (e1 - tb) : L;
#pragma unroll
        for (int sb = 0; sb < L; sb += kDetU) {
            if (sb >= cnt) break;  // (the same for every lane of the group)
            double a[kDetU][kMaxDegree - 1];
#pragma unroll
            for (int u = 0; u < kDetU; ++u) {
                const int r = __shfl(rl, sb + u, L);
                const double* sr = st + (size_t)r * rstride;
#pragma unroll
                for (int t = 1; t < kMaxDegree; ++t)
                    a[u][t - 1] = (act && sb + u < cnt && t < deg) ? sr[(size_t)(t - 1) * k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kDetU; ++u) {
                const double x = __shfl(xl, sb + u, L);
                const double dL = __shfl(dl, sb + u, L);
                double dprev = x;
#pragma unroll
                for (int t = 1; t < kMaxDegree; ++t)
                    if (t < deg) dprev = x * (a[u][t - 1] - p * dprev);
                if (sb + u < cnt) {
                    gp += (dL * lam) * dprev;
                    gw += dL * x;
                }
            }
        }
    }
}

// The segments of one minibatch on a fixed grid: a workgroup walks blocks of kBlock / L consecutive
// segments with a grid stride, one group per segment of at most kDetSeg entries; the longer
// segments of the block are then taken by all its groups together, a piece each, and folded by
// group 0 in piece order.  bi: the minibatch (table-driven: idx[0]).
template <typename T, int L>
__global__ __launch_bounds__(kBlock) void psgd_colgrad_kernel(
    DetPlan pl, const T* __restrict__ rec_x, int bi, const double* __restrict__ Pt,
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
    const size_t rstride = (size_t)n_orders * nst * k;
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
                        double gp, gw;
                        det_piece<T, L>(e0, e1, ln, pl.rec_r, rec_x, dLrow,
                                        state + (size_t)o * nst * k + (act ? cs : 0), rstride, k,
                                        degree - o, act ? lams[cs] : 0.0, act ? Pt[at] : 0.0, act,
                                        gp, gw);
                        if (act) grad_P[at] = gp;
                        if (fit_linear && o == 0 && c == 0 && ln == 0) grad_w[j] = gw;
                    }
            }
        }
        // the long segments of this block (every thread of the workgroup reads the same bounds)
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
                    double tp = 0.0, tw = 0.0;
                    for (int p0 = 0; p0 < npc; p0 += gpb) {
                        const int pc = p0 + grp;
                        double gp = 0.0, gw = 0.0;
                        if (pc < npc) {
                            const int f0 = e0 + pc * kDetSeg;
                            det_piece<T, L>(f0, (e1 - f0 < kDetSeg) ? e1 : f0 + kDetSeg, ln,
                                            pl.rec_r, rec_x, dLrow,
                                            state + (size_t)o * nst * k + (act ? cs : 0), rstride,
                                            k, degree - o, lam, p, act, gp, gw);
                        }
                        __syncthreads();  // group 0 has read the round before
                        red[grp][ln] = gp;
                        if (ln == 0) red[grp][L] = gw;
                        __syncthreads();
                        if (grp == 0)
                            for (int g = 0; g < gpb && p0 + g < npc; ++g) {
                                tp += red[g][ln];
                                tw += red[g][L];
                            }
                    }
                    if (grp == 0 && act) grad_P[at] = tp;
                    if (grp == 0 && fit_linear && o == 0 && c == 0 && ln == 0) grad_w[j] = tw;
                }
        }
    }
}

}  // namespace spfm
