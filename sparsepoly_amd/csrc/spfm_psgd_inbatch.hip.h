// spfm_psgd_inbatch.hip.h -- in-batch softmax gradient of the minibatch solver
// Part of the gfx950 device code of the sparse-FM solvers; see spfm_psgd_lists.hip.h.
//
// A training item is a positive pair (b_q, c_q); the other positives of its minibatch are its
// negatives.  With n positions in the minibatch and, per order of degree M,
//   a_s^M(x + z) = sum_{t=0..M} a_s^t(x) a_s^{M-t}(z)        (disjoint column sets, section 15)
// the logits are s[q, q'] = colconst[q'] + (U V^T)[q, q'] + (a term of the row alone, which the
// softmax cancels and which is never formed):
//   U[q, (t, s)]  = lams_s a_s^t(x_{b_q})                      t = 1..M-1
//   V[q', (t, s)] = a_s^{M-t}(z_{c_q'})
//   colconst[q']  = sum_orders sum_s lams_s a_s^M(z_{c_q'}) + <w, z_{c_q'}>
// R = sum_orders k (M - 1) columns, plus ONE more: U[., R] = 1 and V[., R] = 0.  The logits do not
// see it, and dV[., R] = (G^T U)[., R] = G^T 1 is dcol, the gradient of colconst, for free.  The
// images are row-major (Bpad, Rp): Rp = R + 1 padded to a multiple of 4, Bpad = the batch size
// padded to a multiple of 64, padding zero.  There is no cap on R: the tiles stage their operands
// in chunks of kIntKC columns.
//
// One minibatch is six launches, all of them sized by the batch size and reading the batch
// (pos, B) from the table when there is one (graph replay):
//   inb_tower_kernel      one wave per (position, side): the row's DP per (order, component),
//                         rows gathered through the pair list, duplicates computed per position.
//                         Clears the position's rows of dU / dV and the padding rows.
//   inb_stats_kernel      workgroup (strip, ti): the 64 x 64 logit tiles of row tile ti against
//                         the column tiles of its strip (int_tile_product, the f64 MFMA form);
//                         masking on the accumulator registers; every row's running maximum and
//                         sum (online log-sum-exp) -> one partial per (strip, row).  The diagonal
//                         logit is kept.  Nothing of size n x n is stored, here or below.
//   inb_lse_kernel        merges the strips' partials: mx[q], 1 / z[q], loss_row.
//   inb_grad_tile_kernel  <false>: workgroup (strip, ti, rc) recomputes its tiles, forms
//                         G = softmax - [q' = q] on the registers, passes the G tile through LDS
//                         into operand layout (two halves of 32 columns: the two staging tiles of
//                         the logit product are all the LDS there is) and multiplies it with
//                         columns [64 rc, 64 rc + 64) of the staged V tile: dU = G V, accumulated
//                         over the strip in registers, then f64 atomics into the (Bpad, Rp) buffer.
//                         <true>: the transposed tile V U^T with the roles swapped: dV = G^T U.
//   inb_back_kernel       one L-lane group per (position, side), lane = component: reruns the
//                         row's DP and scatters sum_u cf[u] d a^u / d p_sj with the downward
//                         recurrence of PsgdChunk::grad into sg_gradP / sg_gradw (hardware f64
//                         atomics, where psgd_pair_grad_kernel writes them).
// Masking: column q' != q is left out of row q when c_q' == c_q or b_q' == b_q.
#pragma once
#include "spfm_interactions.hip.h"
#include "spfm_psgd.hip.h"

namespace spfm {

struct InbArgs {
    const int32_t* pairs;  // (m, 2) rows of [X; Z] of the whole epoch, in visiting order
    double *U, *V, *cc;    // (Bpad, Rp) images and colconst (Bpad) of the minibatch
    double *dU, *dV;       // (Bpad, Rp) upstream gradients
    double* part;          // (n_strips, Bpad, 2) running (maximum, sum) per strip and row
    double *mx, *rz, *diag;  // (Bpad) row maximum, 1 / row sum, s[q, q]
    int R, Rp, Bpad;
    int strip_tiles, n_strips;  // column tiles per strip; strips
};

// is column qq part of row q's softmax?  (ids: context and candidate row of each position)
__device__ __forceinline__ bool inb_admitted(int q, int qq, int B, int bq, int cq, int bqq,
                                             int cqq) {
    return q < B && qq < B && (q == qq || (bq != bqq && cq != cqq));
}

template <typename T>
__global__ __launch_bounds__(kBlock) void inb_tower_kernel(
    InbArgs a, long long pos, int B, const PsgdBatch* __restrict__ sched, int* __restrict__ idx,
    const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const T* __restrict__ rval, const double* __restrict__ Pt, const double* __restrict__ w,
    const double* __restrict__ lams, int n_orders, int k, int d, int degree) {
    if (sched) psgd_table_batch(sched, idx, B, pos);
    const int q = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int side = blockIdx.y, lane = threadIdx.x & 63;
    if (q >= a.Bpad) return;  // whole waves leave; no block-level synchronisation below
    double* img = (side == 0 ? a.U : a.V) + (size_t)q * a.Rp;
    double* dimg = (side == 0 ? a.dU : a.dV) + (size_t)q * a.Rp;
    for (int c = lane; c < a.Rp; c += kWave) dimg[c] = 0.0;
    if (q >= B) {  // padding rows: zeros (a tile multiplies them with G = 0)
        for (int c = lane; c < a.Rp; c += kWave) img[c] = 0.0;
        if (side == 1 && lane == 0) a.cc[q] = 0.0;
        return;
    }
    const int row = a.pairs[2 * ((size_t)pos + q) + side];
    const int64_t b = rptr[row], e = rptr[row + 1];
    double acc = 0.0;
    int col0 = 0;
    for (int o = 0; o < n_orders; ++o) {
        const int deg = degree - o;
        for (int s = lane; s < k; s += kWave) {
            const double* Pcol = Pt + (size_t)o * d * k + s;
            double av[kMaxDegree + 1];
            psgd_a_init(av);
            for (int64_t ii = b; ii < e; ++ii) {
                const double x = (double)rval[ii], p = Pcol[(size_t)ridx[ii] * k];
#pragma unroll
                for (int t = kMaxDegree; t >= 1; --t)
                    if (t <= deg) av[t] += av[t - 1] * x * p;
            }
            const double lam = lams[s];
            double top = av[1];
#pragma unroll
            for (int u = 1; u < kMaxDegree; ++u) {
                if (u + 1 == deg) top = av[u + 1];
                if (u < deg) {  // a^u: the context's column t = u, the candidate's t = deg - u
                    const int t = side == 0 ? u : deg - u;
                    img[col0 + (size_t)(t - 1) * k + s] = side == 0 ? lam * av[u] : av[u];
                }
            }
            acc += lam * top;
        }
        col0 += k * (deg - 1);
    }
    for (int c = a.R + lane; c < a.Rp; c += kWave) img[c] = (side == 0 && c == a.R) ? 1.0 : 0.0;
    if (side == 0) return;  // the context's own term cancels under the softmax
    for (int64_t ii = b + lane; ii < e; ii += kWave) acc += (double)rval[ii] * w[ridx[ii]];
    acc = wave_sum(acc);
    if (lane == 0) a.cc[q] = acc;
}

// max / sum over the 16 lanes that hold one accumulator row
__device__ __forceinline__ double inb_row_max(double v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ double inb_row_sum(double v) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// the tiles [t0, t1) of a strip among the Tn live tiles
__device__ __forceinline__ void inb_strip(const InbArgs& a, int strip, int Tn, int& t0, int& t1) {
    t0 = strip * a.strip_tiles;
    t1 = t0 + a.strip_tiles < Tn ? t0 + a.strip_tiles : Tn;
}

// C/D map of the f64 MFMA (spfm_interactions.hip.h): register r of accumulator (ra, cb) of lane l
// in wave 2 wr + wc is row wr 32 + ra 16 + (l >> 4) + 4 r, column wc 32 + cb 16 + (l & 15)
__global__ __launch_bounds__(kBlock) void inb_stats_kernel(InbArgs a, long long pos, int B,
                                                           const PsgdBatch* __restrict__ sched,
                                                           int* __restrict__ idx) {
    __shared__ double sA[kIntTile * kIntLd];
    __shared__ double sB[kIntTile * kIntLd];
    __shared__ double sRed[2][kIntTile][2];
    if (sched) psgd_table_batch(sched, idx, B, pos);
    const int strip = blockIdx.x, ti = blockIdx.y;
    const int Tn = (B + kIntTile - 1) / kIntTile;
    if (ti >= Tn) return;  // the whole workgroup leaves
    int t0, t1;
    inb_strip(a, strip, Tn, t0, t1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int32_t* pr = a.pairs + 2 * (size_t)pos;
    int rb[2][4], rc[2][4];
    double m[2][4], z[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
            rb[ra][r] = q < B ? pr[2 * (size_t)q] : -1;
            rc[ra][r] = q < B ? pr[2 * (size_t)q + 1] : -1;
            m[ra][r] = -INFINITY;
            z[ra][r] = 0.0;
        }
    for (int tj = t0; tj < t1; ++tj) {
        int_v4d acc[2][2];
        int_tile_product(a.U + (size_t)ti * kIntTile * a.Rp, a.V + (size_t)tj * kIntTile * a.Rp,
                         a.Rp, sA, sB, acc);
        int cb_[2], cc_[2];
        double ccv[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int qq = tj * kIntTile + wc * 32 + cb * 16 + l15;
            cb_[cb] = qq < B ? pr[2 * (size_t)qq] : -1;
            cc_[cb] = qq < B ? pr[2 * (size_t)qq + 1] : -1;
            ccv[cb] = a.cc[qq];  // (padded to whole tiles)
        }
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
                double v[2];
                bool in[2];
                double tmax = -INFINITY;
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const int qq = tj * kIntTile + wc * 32 + cb * 16 + l15;
                    v[cb] = acc[ra][cb][r] + ccv[cb];
                    in[cb] = inb_admitted(q, qq, B, rb[ra][r], rc[ra][r], cb_[cb], cc_[cb]);
                    if (q == qq && q < B) a.diag[q] = v[cb];
                    if (in[cb]) tmax = fmax(tmax, v[cb]);
                }
                const double mn = fmax(m[ra][r], inb_row_max(tmax));
                double s = 0.0;
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) s += in[cb] ? exp(v[cb] - mn) : 0.0;
                s = inb_row_sum(s);
                const double scale = m[ra][r] == -INFINITY ? 0.0 : exp(m[ra][r] - mn);
                z[ra][r] = z[ra][r] * scale + s;
                m[ra][r] = mn;
            }
    }
    // the two column halves of a row (waves wc = 0, 1), then one partial per row of the strip
    if (l15 == 0) {
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = wr * 32 + ra * 16 + l4 + 4 * r;
                sRed[wc][rl][0] = m[ra][r];
                sRed[wc][rl][1] = z[ra][r];
            }
    }
    __syncthreads();
    if (threadIdx.x < kIntTile) {
        const int rl = threadIdx.x;
        const double m0 = sRed[0][rl][0], m1 = sRed[1][rl][0];
        const double mm = fmax(m0, m1);
        double zz = 0.0;
        if (m0 != -INFINITY) zz += sRed[0][rl][1] * exp(m0 - mm);
        if (m1 != -INFINITY) zz += sRed[1][rl][1] * exp(m1 - mm);
        double* dst = a.part + ((size_t)strip * a.Bpad + (size_t)ti * kIntTile + rl) * 2;
        dst[0] = mm;
        dst[1] = zz;
    }
}

// one thread per position: the strips' partials -> mx, 1 / z and the position's loss
static __global__ __launch_bounds__(kBlock) void inb_lse_kernel(
    InbArgs a, long long pos, int B, const PsgdBatch* __restrict__ sched, int* __restrict__ idx,
    double* __restrict__ loss_row) {
    if (sched) psgd_table_batch(sched, idx, B, pos);
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.Bpad) return;
    if (q >= B) {
        a.mx[q] = 0.0;
        a.rz[q] = 0.0;
        return;
    }
    const int Tn = (B + kIntTile - 1) / kIntTile;
    const int ns = (Tn + a.strip_tiles - 1) / a.strip_tiles;  // strips that hold a live tile
    double mm = -INFINITY;
    for (int s = 0; s < ns; ++s) mm = fmax(mm, a.part[((size_t)s * a.Bpad + q) * 2]);
    double zz = 0.0;
    for (int s = 0; s < ns; ++s) {
        const double ms = a.part[((size_t)s * a.Bpad + q) * 2];
        if (ms != -INFINITY) zz += a.part[((size_t)s * a.Bpad + q) * 2 + 1] * exp(ms - mm);
    }
    a.mx[q] = mm;
    a.rz[q] = 1.0 / zz;
    loss_row[(size_t)pos + q] = (mm - a.diag[q]) + log(zz);  // the diagonal is always admitted
}

// TRANS = false: rows are the positions q of tile `own`, columns the q' of the strip's tiles;
// dU[q, .] += sum_q' G[q, q'] V[q', .].  TRANS = true: rows are the q' of tile `own`, columns the
// q; dV[q', .] += sum_q G[q, q'] U[q, .].
template <bool TRANS>
__global__ __launch_bounds__(kBlock) void inb_grad_tile_kernel(InbArgs a, long long pos, int B,
                                                               const PsgdBatch* __restrict__ sched,
                                                               int* __restrict__ idx) {
    __shared__ double sA[kIntTile * kIntLd];
    __shared__ double sB[kIntTile * kIntLd];
    static_assert(kIntKC == 32 && kIntTile == 64, "the G tile goes through LDS in two halves");
    if (sched) psgd_table_batch(sched, idx, B, pos);
    const int strip = blockIdx.x, own = blockIdx.y, c0 = blockIdx.z * kIntTile;
    const int Tn = (B + kIntTile - 1) / kIntTile;
    int t0, t1;
    inb_strip(a, strip, Tn, t0, t1);
    if (own >= Tn || t0 >= t1) return;  // the whole workgroup leaves
    const double* Aimg = TRANS ? a.V : a.U;  // the rows' image
    const double* Oimg = TRANS ? a.U : a.V;  // the columns' image: logit operand and G's factor
    double* Dout = TRANS ? a.dV : a.dU;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int32_t* pr = a.pairs + 2 * (size_t)pos;
    // per row of the lane: ids, and what the row's side gives a logit (TRANS: colconst; else the
    // softmax's maximum and 1 / sum)
    int rb[2][4], rc[2][4];
    double r0[2][4], r1[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = own * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
            rb[ra][r] = i < B ? pr[2 * (size_t)i] : -1;
            rc[ra][r] = i < B ? pr[2 * (size_t)i + 1] : -1;
            r0[ra][r] = TRANS ? a.cc[i] : a.mx[i];
            r1[ra][r] = TRANS ? 0.0 : a.rz[i];
        }
    int_v4d out[2][2];
    int_acc_zero(out);
    for (int to = t0; to < t1; ++to) {
        int_v4d acc[2][2];
        int_tile_product(Aimg + (size_t)own * kIntTile * a.Rp, Oimg + (size_t)to * kIntTile * a.Rp,
                         a.Rp, sA, sB, acc);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int j = to * kIntTile + wc * 32 + cb * 16 + l15;
            const int jb = j < B ? pr[2 * (size_t)j] : -1, jc = j < B ? pr[2 * (size_t)j + 1] : -1;
            const double j0 = TRANS ? a.mx[j] : a.cc[j], j1 = TRANS ? a.rz[j] : 0.0;
#pragma unroll
            for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = own * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
                    // (admission is symmetric in the two positions)
                    const bool in = inb_admitted(i, j, B, rb[ra][r], rc[ra][r], jb, jc);
                    const double cc = TRANS ? r0[ra][r] : j0, mx = TRANS ? j0 : r0[ra][r];
                    const double rz = TRANS ? j1 : r1[ra][r];
                    const double g = exp((acc[ra][cb][r] + cc) - mx) * rz - (i == j ? 1.0 : 0.0);
                    acc[ra][cb][r] = in ? g : 0.0;
                }
        }
        // G (64 x 64) against columns [c0, c0 + 64) of the columns' image, 32 inner positions at
        // a time: sA = G[., 32 h ..], sB = image^T
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __syncthreads();  // the last MFMA step has read both tiles
            if (wc == h) {
#pragma unroll
                for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            sA[(wr * 32 + ra * 16 + l4 + 4 * r) * kIntLd + cb * 16 + l15] =
                                acc[ra][cb][r];
            }
#pragma unroll
            for (int i = 0; i < kIntTile * kIntKC / kBlock; ++i) {
                const int e = tid + i * kBlock, c = e % kIntTile, kk = e / kIntTile;
                const size_t prow = (size_t)to * kIntTile + h * kIntKC + kk;
                sB[c * kIntLd + kk] = (c0 + c < a.Rp) ? Oimg[prow * a.Rp + c0 + c] : 0.0;
            }
            __syncthreads();
            int_mfma_chunk<false>(sA, sB, kIntKC, nullptr, out);
        }
    }
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = own * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
                const int c = c0 + wc * 32 + cb * 16 + l15;
                if (i < B && c < a.Rp) unsafeAtomicAdd(&Dout[(size_t)i * a.Rp + c], out[ra][cb][r]);
            }
}

// sum_u cf[u] d a^u / d p_sj over a chunk: a^v without entry j by the downward recurrence
// e_0 = 1, e_v = a[v] - p_j x_j e_{v-1}; d a^u / d p_sj = x_j e_{u-1}
template <typename T, int L>
__device__ __forceinline__ void inb_chunk_grad(const PsgdChunk<T, L>& ch, const double* a,
                                               const double* cf, int deg,
                                               double* __restrict__ Gcol, int k, bool act) {
#pragma unroll
    for (int u = 0; u < kPsgdRC; ++u) {
        const int j = ch.col(u);
        const double x = ch.val(u);
        double e = 1.0, g = cf[1];
#pragma unroll
        for (int v = 1; v < kMaxDegree; ++v)
            if (v < deg) {
                e = a[v] - ch.p[u] * x * e;
                g += cf[v + 1] * e;
            }
        if (act && u < ch.cnt) unsafeAtomicAdd(&Gcol[(size_t)j * k], x * g);
    }
}

// One L-lane group per (position, side).  side 0: the context row with cf[t] = lams_s dU[q, (t, s)];
// side 1: the candidate row with cf[M - t] = dV[q', (t, s)], cf[M] = lams_s dcol[q'], and
// grad_w[j] += dcol[q'] z_j.
template <typename T, int L>
__global__ __launch_bounds__(kBlock) void inb_back_kernel(
    InbArgs a, long long pos, int B, const PsgdBatch* __restrict__ sched, int* __restrict__ idx,
    const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const T* __restrict__ rval, const double* __restrict__ Pt, const double* __restrict__ lams,
    int n_orders, int k, int d, int degree, int fit_linear, double* __restrict__ grad_P,
    double* __restrict__ grad_w) {
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    const int r = blockIdx.x * gpb + grp, side = blockIdx.y;
    if (sched) psgd_table_batch(sched, idx, B, pos);
    if (r >= B) return;  // whole groups leave; no block-level synchronisation below
    const int row = a.pairs[2 * ((size_t)pos + r) + side];
    const int64_t lo = rptr[row], hi = rptr[row + 1];
    const double* dimg = (side == 0 ? a.dU : a.dV) + (size_t)r * a.Rp;
    const double dcol = side == 0 ? 0.0 : dimg[a.R];
    if (side == 1 && fit_linear)
        for (int64_t e = lo + ln; e < hi; e += L)
            unsafeAtomicAdd(&grad_w[ridx[e]], dcol * (double)rval[e]);
    if (hi == lo) return;
    const int C = (k + L - 1) / L;
    PsgdChunk<T, L> ch;
    double av[kMaxDegree + 1], cf[kMaxDegree + 1];
    int col0 = 0;
    for (int o = 0; o < n_orders; ++o) {
        const int deg = degree - o;
        for (int c = 0; c < C; ++c) {
            const int s = c * L + ln;
            const bool act = s < k;
            const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
            double* Gcol = grad_P + (size_t)o * d * k + (act ? s : 0);
            const double lam = act ? lams[s] : 0.0;
            cf[0] = 0.0;
#pragma unroll
            for (int u = 1; u <= kMaxDegree; ++u) {
                double v = 0.0;
                if (u < deg && act) {
                    const int t = side == 0 ? u : deg - u;
                    v = dimg[col0 + (size_t)(t - 1) * k + s];
                    if (side == 0) v *= lam;
                } else if (u == deg) {
                    v = dcol * lam;
                }
                cf[u] = v;
            }
            psgd_a_init(av);
            psgd_row_dp(ch, lo, hi, ln, ridx, rval, Pcol, k, act, deg, av);
            for (int64_t tb = lo; tb < hi; tb += kPsgdRC) {
                ch.load_entries(tb, hi, ln, ridx, rval);
                ch.load_p(Pcol, k, act);
                inb_chunk_grad(ch, av, cf, deg, Gcol, k, act);
            }
        }
        col0 += k * (deg - 1);
    }
}

}  // namespace spfm
