// spfm_psgd_full.hip.h -- full-catalogue softmax gradient of the minibatch solver
// Part of the gfx950 device code of the sparse-FM solvers; see spfm_psgd_inbatch.hip.h, whose
// towers, MFMA tile product and per-row gradient recurrence this unit calls.
//
// A training item is a positive pair (b_q, c_q); EVERY candidate c < C that the context has not
// interacted with is a negative.  The logits of a minibatch of n positions are n x C,
//   s[q, c] = colconst[c] + (U Vc^T)[q, c]
// with U (Bpad, Rp) the context tower of section 19h (gathered through the pair list, its last
// live column R all ones) and Vc (Cpad, Rp) the CATALOGUE tower: row c is candidate row B0 + c of
// the image, formed once per minibatch without a pair list.  Cpad = C padded to a multiple of 64.
// Candidate c is admitted to row q iff c == c_q or c is not in F[b_q], F the resident forbidden
// CSR of the sampler (sorted rows, candidate numbering).
//
// Masking never stores anything of size n x C nor a table of (n, C / 64) words.  For one 64 x 64
// tile, 64 lanes each take one position, walk their slice of F[b_q] that falls inside the tile's
// 64 candidates and leave one 64-bit word in LDS (512 bytes); every accumulator register then
// tests its bit.  Catalogue tiles of a strip ascend, so a position's place in F[b_q] is found by
// one binary search at the strip's first tile and only moves forward afterwards (full_mask_walk).
//
// One minibatch is eight launches, reading the batch (pos, B) from the table on graph replay:
//   inb_tower_kernel       (grid of side 0 alone) the context tower U; clears dU
//   full_tower_kernel      one wave per catalogue row: Vc, colconst; clears dVc; padding rows 0
//   full_stats_kernel      workgroup (catalogue strip, row tile): online log-sum-exp per row over
//                          the strip's tiles -> one (max, sum) partial per (strip, row); the lane
//                          that owns (q, c_q) stores the positive's logit
//   full_lse_kernel        merges the strips' partials: mx[q], 1 / z[q], loss_row
//   full_grad_tile_kernel  <false>: own = a row tile, strips over catalogue tiles: dU = G Vc,
//                          accumulated over the strip in registers.  <true>: own = a catalogue
//                          tile, strips over row tiles: dVc = G^T U, whose column R is dcol = G^T 1.
//                          Both recompute the logit tile, form G = softmax - [c == c_q] on the
//                          registers, pass it through LDS in two halves of 32 and multiply it with
//                          64 columns of the staged image (section 19h).  Strips meet in f64
//                          atomics.
//   inb_back_kernel        (grid of side 0 alone) the context rows' gradient from dU
//   full_back_kernel       one L-lane group per catalogue row: the row's DP and inb_chunk_grad
//                          with cf[M - t] = dVc[c, (t, s)], cf[M] = lams_s dcol[c];
//                          grad_w[j] += dcol[c] z_j
#pragma once
// inb_stats_kernel is that header's one kernel with external linkage (neither a template nor
// static), so a second unit that includes it would define the symbol again.  This unit never
// launches it; its unused copy gets a name of its own.
#define inb_stats_kernel inb_stats_kernel_copy_of_full_unit
#include "spfm_psgd_inbatch.hip.h"
#undef inb_stats_kernel

namespace spfm {

struct FullArgs {
    const int32_t* pairs;  // (m, 2) rows of [X; Z] of the whole epoch, in visiting order
    const int64_t* fptr;   // forbidden CSR over the contexts, candidate numbering, rows sorted
    const int32_t* fidx;
    double *U, *dU;         // (Bpad, Rp) context tower of the minibatch and its gradient
    double *Vc, *dVc, *cc;  // (Cpad, Rp) catalogue tower, its gradient; colconst (Cpad)
    double* part;           // (st_strips, Bpad, 2) running (maximum, sum) per strip and row
    double *mx, *rz, *spos;  // (Bpad) row maximum, 1 / row sum, s[q, c_q]
    int R, Rp, Bpad, Cpad;
    int B0, C;               // first candidate row of the image; live candidates
    int st_tiles, st_strips;  // statistics pass: catalogue tiles per strip, strips
    int gu_tiles, gu_strips;  // dU pass: catalogue tiles per strip, strips
    int gv_tiles, gv_strips;  // dVc pass: row tiles per strip, strips
};

// the context-side view the two kernels of section 19h need (their side 0 reads nothing else)
static inline InbArgs full_ctx_view(const FullArgs& a) {
    InbArgs v{};
    v.pairs = a.pairs;
    v.U = a.U;
    v.dU = a.dU;
    v.R = a.R;
    v.Rp = a.Rp;
    v.Bpad = a.Bpad;
    return v;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void full_tower_kernel(
    FullArgs a, const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const T* __restrict__ rval, const double* __restrict__ Pt, const double* __restrict__ w,
    const double* __restrict__ lams, int n_orders, int k, int d, int degree) {
    const int c = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= a.Cpad) return;  // whole waves leave; no block-level synchronisation below
    double* img = a.Vc + (size_t)c * a.Rp;
    double* dimg = a.dVc + (size_t)c * a.Rp;
    for (int i = lane; i < a.Rp; i += kWave) dimg[i] = 0.0;
    if (c >= a.C) {  // padding rows: zeros (their columns are never admitted)
        for (int i = lane; i < a.Rp; i += kWave) img[i] = 0.0;
        if (lane == 0) a.cc[c] = 0.0;
        return;
    }
    const int64_t b = rptr[a.B0 + c], e = rptr[a.B0 + c + 1];
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
            double top = av[1];
#pragma unroll
            for (int u = 1; u < kMaxDegree; ++u) {
                if (u + 1 == deg) top = av[u + 1];
                if (u < deg) img[col0 + (size_t)(deg - u - 1) * k + s] = av[u];  // column t = deg - u
            }
            acc += lams[s] * top;
        }
        col0 += k * (deg - 1);
    }
    for (int i = a.R + lane; i < a.Rp; i += kWave) img[i] = 0.0;
    for (int64_t ii = b + lane; ii < e; ii += kWave) acc += (double)rval[ii] * w[ridx[ii]];
    acc = wave_sum(acc);
    if (lane == 0) a.cc[c] = acc;
}

// first entry of the sorted slice idx[lo, hi) that is >= key
__device__ __forceinline__ int64_t full_lower_bound(const int32_t* __restrict__ idx, int64_t lo,
                                                    int64_t hi, int key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the forbidden candidates of [c0, c0 + 64) as bits, walking the cursor forward to the first
// entry beyond them
__device__ __forceinline__ unsigned long long full_mask_walk(const int32_t* __restrict__ fidx,
                                                             int64_t& cur, int64_t end, int c0) {
    unsigned long long word = 0ull;
    while (cur < end) {
        const int f = fidx[cur] - c0;
        if (f >= kIntTile) break;
        word |= 1ull << f;
        ++cur;
    }
    return word;
}

// is candidate c (bit `bit` of the row's word) part of row q's softmax?  cq: the row's positive
__device__ __forceinline__ bool full_admitted(bool row_live, int c, int C, int cq,
                                              unsigned long long word, int bit) {
    return row_live && c < C && (c == cq || !((word >> bit) & 1ull));
}

// C/D map of the f64 MFMA as in inb_stats_kernel: register r of accumulator (ra, cb) of lane l in
// wave 2 wr + wc is row wr 32 + ra 16 + (l >> 4) + 4 r, column wc 32 + cb 16 + (l & 15)
static __global__ __launch_bounds__(kBlock) void full_stats_kernel(
    FullArgs a, long long pos, int B, const PsgdBatch* __restrict__ sched, int* __restrict__ idx) {
    __shared__ double sA[kIntTile * kIntLd];
    __shared__ double sB[kIntTile * kIntLd];
    __shared__ double sRed[2][kIntTile][2];
    __shared__ unsigned long long sMask[kIntTile];
    if (sched) psgd_table_batch(sched, idx, B, pos);
    const int strip = blockIdx.x, ti = blockIdx.y;
    if (ti * kIntTile >= B) return;  // the whole workgroup leaves
    const int Tc = a.Cpad / kIntTile;
    const int t0 = strip * a.st_tiles, t1 = t0 + a.st_tiles < Tc ? t0 + a.st_tiles : Tc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int32_t* pr = a.pairs + 2 * (size_t)pos;
    // wave 0: lane = position of the row tile; its cursor into F[b_q]
    int64_t cur = 0, end = 0;
    if (tid < kIntTile && ti * kIntTile + tid < B) {
        const int bq = pr[2 * (size_t)(ti * kIntTile + tid)];
        end = a.fptr[bq + 1];
        cur = full_lower_bound(a.fidx, a.fptr[bq], end, t0 * kIntTile);
    }
    int rc[2][4];
    double m[2][4], z[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
            rc[ra][r] = q < B ? pr[2 * (size_t)q + 1] - a.B0 : -1;
            m[ra][r] = -INFINITY;
            z[ra][r] = 0.0;
        }
    for (int tj = t0; tj < t1; ++tj) {
        unsigned long long word = 0ull;
        if (tid < kIntTile) word = full_mask_walk(a.fidx, cur, end, tj * kIntTile);
        __syncthreads();  // the last epilogue has read the words
        if (tid < kIntTile) sMask[tid] = word;
        int_v4d acc[2][2];
        int_tile_product(a.U + (size_t)ti * kIntTile * a.Rp, a.Vc + (size_t)tj * kIntTile * a.Rp,
                         a.Rp, sA, sB, acc);  // (its barriers publish the words)
        double ccv[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) ccv[cb] = a.cc[tj * kIntTile + wc * 32 + cb * 16 + l15];
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = wr * 32 + ra * 16 + l4 + 4 * r, q = ti * kIntTile + rl;
                const unsigned long long wq = sMask[rl];
                double v[2];
                bool in[2];
                double tmax = -INFINITY;
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const int bit = wc * 32 + cb * 16 + l15, c = tj * kIntTile + bit;
                    v[cb] = acc[ra][cb][r] + ccv[cb];
                    in[cb] = full_admitted(q < B, c, a.C, rc[ra][r], wq, bit);
                    if (q < B && c == rc[ra][r]) a.spos[q] = v[cb];
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
    if (tid < kIntTile) {
        const double m0 = sRed[0][tid][0], m1 = sRed[1][tid][0];
        const double mm = fmax(m0, m1);
        double zz = 0.0;
        if (m0 != -INFINITY) zz += sRed[0][tid][1] * exp(m0 - mm);
        if (m1 != -INFINITY) zz += sRed[1][tid][1] * exp(m1 - mm);
        double* dst = a.part + ((size_t)strip * a.Bpad + (size_t)ti * kIntTile + tid) * 2;
        dst[0] = mm;
        dst[1] = zz;
    }
}

// one thread per position: the catalogue strips' partials -> mx, 1 / z and the position's loss
// (every strip holds a tile, and the strip of c_q admits it: the sum is positive)
static __global__ __launch_bounds__(kBlock) void full_lse_kernel(
    FullArgs a, long long pos, int B, const PsgdBatch* __restrict__ sched, int* __restrict__ idx,
    double* __restrict__ loss_row) {
    if (sched) psgd_table_batch(sched, idx, B, pos);
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= a.Bpad) return;
    if (q >= B) {
        a.mx[q] = 0.0;
        a.rz[q] = 0.0;
        return;
    }
    double mm = -INFINITY;
    for (int s = 0; s < a.st_strips; ++s) mm = fmax(mm, a.part[((size_t)s * a.Bpad + q) * 2]);
    double zz = 0.0;
    for (int s = 0; s < a.st_strips; ++s) {
        const double ms = a.part[((size_t)s * a.Bpad + q) * 2];
        if (ms != -INFINITY) zz += a.part[((size_t)s * a.Bpad + q) * 2 + 1] * exp(ms - mm);
    }
    a.mx[q] = mm;
    a.rz[q] = 1.0 / zz;
    loss_row[(size_t)pos + q] = (mm - a.spos[q]) + log(zz);
}

// TRANS = false: rows are the positions q of row tile `own`, columns the candidates of the
// strip's catalogue tiles; dU[q, .] += sum_c G[q, c] Vc[c, .].  TRANS = true: rows are the
// candidates of catalogue tile `own`, columns the positions of the strip's row tiles;
// dVc[c, .] += sum_q G[q, c] U[q, .].  The mask words belong to the positions either way: of the
// own tile with a forward cursor (false), of the walked tile by a search per tile (true).
template <bool TRANS>
__global__ __launch_bounds__(kBlock) void full_grad_tile_kernel(
    FullArgs a, long long pos, int B, const PsgdBatch* __restrict__ sched, int* __restrict__ idx) {
    __shared__ double sA[kIntTile * kIntLd];
    __shared__ double sB[kIntTile * kIntLd];
    __shared__ unsigned long long sMask[kIntTile];
    static_assert(kIntKC == 32 && kIntTile == 64, "the G tile goes through LDS in two halves");
    if (sched) psgd_table_batch(sched, idx, B, pos);
    const int strip = blockIdx.x, own = blockIdx.y, c0 = blockIdx.z * kIntTile;
    const int Tn = (B + kIntTile - 1) / kIntTile, Tc = a.Cpad / kIntTile;
    const int st = TRANS ? a.gv_tiles : a.gu_tiles, To = TRANS ? Tn : Tc;
    const int t0 = strip * st, t1 = t0 + st < To ? t0 + st : To;
    if (own >= (TRANS ? Tc : Tn) || t0 >= t1) return;  // the whole workgroup leaves
    const double* Aimg = TRANS ? a.Vc : a.U;  // the rows' image
    const double* Oimg = TRANS ? a.U : a.Vc;  // the columns' image: logit operand and G's factor
    double* Dout = TRANS ? a.dVc : a.dU;
    const int nrows = TRANS ? a.C : B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const int32_t* pr = a.pairs + 2 * (size_t)pos;
    int64_t cur = 0, end = 0;  // !TRANS, wave 0: the cursor of position own * 64 + lane
    if (!TRANS && tid < kIntTile && own * kIntTile + tid < B) {
        const int bq = pr[2 * (size_t)(own * kIntTile + tid)];
        end = a.fptr[bq + 1];
        cur = full_lower_bound(a.fidx, a.fptr[bq], end, t0 * kIntTile);
    }
    // per row of the lane (TRANS: colconst; else the positive, the maximum and 1 / sum)
    int rq[2][4];
    double r0[2][4], r1[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = own * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
            rq[ra][r] = (!TRANS && i < B) ? pr[2 * (size_t)i + 1] - a.B0 : -1;
            r0[ra][r] = TRANS ? a.cc[i] : a.mx[i];
            r1[ra][r] = TRANS ? 0.0 : a.rz[i];
        }
    int_v4d out[2][2];
    int_acc_zero(out);
    for (int to = t0; to < t1; ++to) {
        if (tid < kIntTile) {  // (the barriers of the last tile's G passes lie behind its reads)
            unsigned long long word = 0ull;
            if (TRANS) {
                const int q = to * kIntTile + tid;
                if (q < B) {
                    const int bq = pr[2 * (size_t)q];
                    const int64_t e = a.fptr[bq + 1];
                    int64_t cu = full_lower_bound(a.fidx, a.fptr[bq], e, own * kIntTile);
                    word = full_mask_walk(a.fidx, cu, e, own * kIntTile);
                }
            } else {
                word = full_mask_walk(a.fidx, cur, end, to * kIntTile);
            }
            sMask[tid] = word;
        }
        int_v4d acc[2][2];
        int_tile_product(Aimg + (size_t)own * kIntTile * a.Rp, Oimg + (size_t)to * kIntTile * a.Rp,
                         a.Rp, sA, sB, acc);  // (its barriers publish the words)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int jl = wc * 32 + cb * 16 + l15, j = to * kIntTile + jl;
            const int jq = (TRANS && j < B) ? pr[2 * (size_t)j + 1] - a.B0 : -1;
            const double j0 = TRANS ? a.mx[j] : a.cc[j], j1 = TRANS ? a.rz[j] : 0.0;
            const unsigned long long wj = TRANS ? sMask[jl] : 0ull;
#pragma unroll
            for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int il = wr * 32 + ra * 16 + l4 + 4 * r, i = own * kIntTile + il;
                    const int q = TRANS ? j : i, c = TRANS ? i : j, cq = TRANS ? jq : rq[ra][r];
                    const unsigned long long wq = TRANS ? wj : sMask[il];
                    const bool in = full_admitted(q < B, c, a.C, cq, wq, TRANS ? il : jl);
                    const double cc = TRANS ? r0[ra][r] : j0, mx = TRANS ? j0 : r0[ra][r];
                    const double rz = TRANS ? j1 : r1[ra][r];
                    const double g = exp((acc[ra][cb][r] + cc) - mx) * rz - (c == cq ? 1.0 : 0.0);
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
                if (i < nrows && c < a.Rp)
                    unsafeAtomicAdd(&Dout[(size_t)i * a.Rp + c], out[ra][cb][r]);
            }
}

// One L-lane group per catalogue row, lane = component: the candidate side of inb_back_kernel
// without a pair list.
template <typename T, int L>
__global__ __launch_bounds__(kBlock) void full_back_kernel(
    FullArgs a, const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
    const T* __restrict__ rval, const double* __restrict__ Pt, const double* __restrict__ lams,
    int n_orders, int k, int d, int degree, int fit_linear, double* __restrict__ grad_P,
    double* __restrict__ grad_w) {
    constexpr int gpb = kBlock / L;
    const int grp = threadIdx.x / L, ln = threadIdx.x % L;
    const int c = blockIdx.x * gpb + grp;
    if (c >= a.C) return;  // whole groups leave; no block-level synchronisation below
    const int64_t lo = rptr[a.B0 + c], hi = rptr[a.B0 + c + 1];
    const double* dimg = a.dVc + (size_t)c * a.Rp;
    const double dcol = dimg[a.R];
    if (fit_linear)
        for (int64_t e = lo + ln; e < hi; e += L)
            unsafeAtomicAdd(&grad_w[ridx[e]], dcol * (double)rval[e]);
    if (hi == lo) return;
    const int NC = (k + L - 1) / L;
    PsgdChunk<T, L> ch;
    double av[kMaxDegree + 1], cf[kMaxDegree + 1];
    int col0 = 0;
    for (int o = 0; o < n_orders; ++o) {
        const int deg = degree - o;
        for (int cn = 0; cn < NC; ++cn) {
            const int s = cn * L + ln;
            const bool act = s < k;
            const double* Pcol = Pt + (size_t)o * d * k + (act ? s : 0);
            double* Gcol = grad_P + (size_t)o * d * k + (act ? s : 0);
            const double lam = act ? lams[s] : 0.0;
            cf[0] = 0.0;
#pragma unroll
            for (int u = 1; u <= kMaxDegree; ++u) {
                double v = 0.0;
                if (u < deg && act)
                    v = dimg[col0 + (size_t)(deg - u - 1) * k + s];  // column t = deg - u
                else if (u == deg)
                    v = dcol * lam;
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
