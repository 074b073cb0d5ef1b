// spfm_objective.hip.h -- penalty terms and sparsity counts of one parameter block, held-out
// loss sums (spfm_objective_terms / spfm_eval_loss, include/spfm.h)
// Part of the gfx950 device code of the sparse-FM proximal CD core; see DESIGN.md section 13.
//
// The block P_o (k components x d features) is read ONCE, in whichever layout is live: element
// (s, j) lives at base[s * ss + j * sj] -- (ss, sj) = (d, 1) for the (k,d) image the pcd passes
// keep, (1, k) for the (d,k) image of pbcd / psgd.  Which element meets which partial result is
// decided by (s, j) alone, so both layouts give the same bits.
//
// Stage 1 (obj_block_kernel): workgroup c owns the features [c * kObjTile, (c+1) * kObjTile),
// thread t the features c * kObjTile + t + f * kBlock (f < kObjF).  For every component it
// reduces its features' |p| to one record -- sum of squares, absolute sum, non-zero count,
// prod (1 + v) and e_1..e_M of the values -- and, after the last component, the same record for
// the feature norms n_j = sqrt(sum_s p_sj^2) as pseudo-component k (its count = features with any
// non-zero entry).  Stage 2 (obj_finish_kernel, one workgroup) combines the records of all
// workgroups per component and forms the eight output slots.
//
// e_0..e_M of a set of values are the coefficients of prod (1 + v t) truncated at t^M.  Truncated
// polynomial multiplication is associative and commutative, so every thread runs the reference's
// in-place recurrence (omegati.py:62-74) over its own values and the partial products are
// multiplied in a fixed tree: lanes (shuffle-down, lane 0 holds the result), the four waves in
// order, then in stage 2 a contiguous run of workgroups per lane, lanes again.  All operands are
// non-negative: no cancellation.  A product with a zero factor is skipped, so an overflowed
// coefficient never meets 0 * inf (the sequential host recurrence meets it only where a true
// zero follows an overflow).
#pragma once
#include "spfm_common.hip.h"

namespace spfm {

constexpr int kObjF = 2;                      // features per thread
constexpr int kObjTile = kBlock * kObjF;      // features per workgroup
constexpr int kObjRec = 4 + kMaxDegree;       // doubles per record
enum { OBJ_SUMSQ = 0, OBJ_ABS = 1, OBJ_NNZ = 2, OBJ_PROD = 3, OBJ_E1 = 4 };

// partial result over a set of non-negative values; e[t - 1] = e_t
template <int M>
struct ObjPart {
    double sumsq, abs, nnz, prod;
    double e[M > 0 ? M : 1];
};

template <int M>
__device__ __forceinline__ void obj_init(ObjPart<M>& a) {
    a.sumsq = a.abs = a.nnz = 0.0;
    a.prod = 1.0;
#pragma unroll
    for (int t = 0; t < (M > 0 ? M : 1); ++t) a.e[t] = 0.0;
}

__device__ __forceinline__ double obj_mul(double a, double b) {
    return (a == 0.0 || b == 0.0) ? 0.0 : a * b;
}

// one more value v >= 0 with square `sq` and non-zero flag `nz`
template <int M>
__device__ __forceinline__ void obj_push(ObjPart<M>& a, double v, double sq, double nz) {
    a.sumsq += sq;
    a.abs += v;
    a.nnz += nz;
    a.prod *= 1.0 + v;
    if constexpr (M > 0) {
#pragma unroll
        for (int t = M; t >= 2; --t) a.e[t - 1] += obj_mul(a.e[t - 2], v);
        a.e[0] += v;
    }
}

// a <- a (x) b: sums add, products multiply, polynomials convolve (truncated at t^M)
template <int M>
__device__ __forceinline__ void obj_combine(ObjPart<M>& a, const ObjPart<M>& b) {
    a.sumsq += b.sumsq;
    a.abs += b.abs;
    a.nnz += b.nnz;
    a.prod *= b.prod;
    if constexpr (M > 0) {
        double c[M];
#pragma unroll
        for (int t = 1; t <= M; ++t) {
            double acc = a.e[t - 1];                       // a_t * b_0
#pragma unroll
            for (int i = t - 1; i >= 1; --i) acc += obj_mul(a.e[i - 1], b.e[t - i - 1]);
            acc += b.e[t - 1];                             // a_0 * b_t
            c[t - 1] = acc;
        }
#pragma unroll
        for (int t = 0; t < M; ++t) a.e[t] = c[t];
    }
}

template <int M>
__device__ __forceinline__ void obj_shfl_down(ObjPart<M>& a, int off) {
    ObjPart<M> b;
    b.sumsq = __shfl_down(a.sumsq, off, kWave);
    b.abs = __shfl_down(a.abs, off, kWave);
    b.nnz = __shfl_down(a.nnz, off, kWave);
    b.prod = __shfl_down(a.prod, off, kWave);
#pragma unroll
    for (int t = 0; t < (M > 0 ? M : 1); ++t) b.e[t] = __shfl_down(a.e[t], off, kWave);
    obj_combine<M>(a, b);  // lanes whose partner is out of range combine garbage; lane 0 never does
}

// lane 0 of the wave receives the product of the 64 lanes' parts, in lane order
template <int M>
__device__ __forceinline__ void obj_wave_reduce(ObjPart<M>& a) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) obj_shfl_down<M>(a, off);
}

template <int M>
__device__ __forceinline__ void obj_store(const ObjPart<M>& a, double* __restrict__ rec) {
    rec[OBJ_SUMSQ] = a.sumsq;
    rec[OBJ_ABS] = a.abs;
    rec[OBJ_NNZ] = a.nnz;
    rec[OBJ_PROD] = a.prod;
#pragma unroll
    for (int t = 0; t < kMaxDegree; ++t) rec[OBJ_E1 + t] = (t < M) ? a.e[t] : 0.0;
}

template <int M>
__device__ __forceinline__ void obj_load(ObjPart<M>& a, const double* __restrict__ rec) {
    a.sumsq = rec[OBJ_SUMSQ];
    a.abs = rec[OBJ_ABS];
    a.nnz = rec[OBJ_NNZ];
    a.prod = rec[OBJ_PROD];
#pragma unroll
    for (int t = 0; t < (M > 0 ? M : 1); ++t) a.e[t] = (t < M) ? rec[OBJ_E1 + t] : 0.0;
}

// the workgroup's record of one (pseudo-)component: waves in order, written by thread 0
template <int M>
__device__ __forceinline__ void obj_block_reduce(ObjPart<M>& a, double* red /*[4][kObjRec]*/,
                                                 double* __restrict__ rec) {
    obj_wave_reduce<M>(a);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) obj_store<M>(a, red + wave * kObjRec);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) {
            ObjPart<M> b;
            obj_load<M>(b, red + w * kObjRec);
            obj_combine<M>(a, b);
        }
        obj_store<M>(a, rec);
    }
}

// stage 1: rec[(blockIdx.x * (k + 1) + s) * kObjRec ..], s = k: the feature norms
template <int M>
__global__ __launch_bounds__(kBlock) void obj_block_kernel(const double* __restrict__ base,
                                                           int64_t ss, int64_t sj, int k, int d,
                                                           double* __restrict__ rec) {
    __shared__ double red[(kBlock / kWave) * kObjRec];
    const int64_t j0 = (int64_t)blockIdx.x * kObjTile + threadIdx.x;
    double nsq[kObjF], any[kObjF];
#pragma unroll
    for (int f = 0; f < kObjF; ++f) nsq[f] = any[f] = 0.0;
    double* out = rec + (size_t)blockIdx.x * (k + 1) * kObjRec;
    for (int s = 0; s < k; ++s) {
        ObjPart<M> a;
        obj_init<M>(a);
#pragma unroll
        for (int f = 0; f < kObjF; ++f) {
            const int64_t j = j0 + (int64_t)f * kBlock;
            const double p = (j < d) ? base[s * ss + j * sj] : 0.0;
            const double v = fabs(p), sq = p * p, nz = (p != 0.0) ? 1.0 : 0.0;
            nsq[f] += sq;
            if (p != 0.0) any[f] = 1.0;
            obj_push<M>(a, v, sq, nz);
        }
        obj_block_reduce<M>(a, red, out + (size_t)s * kObjRec);
    }
    ObjPart<M> a;
    obj_init<M>(a);
#pragma unroll
    for (int f = 0; f < kObjF; ++f) obj_push<M>(a, sqrt(nsq[f]), nsq[f], any[f]);
    obj_block_reduce<M>(a, red, out + (size_t)k * kObjRec);
}

// stage 2, ONE workgroup: wave w combines the nblk records of the components w, w + 4, ...
// (lane l a contiguous run of workgroups, then the lane tree) into fin[s]; thread 0 then adds
// the components up in order and writes the eight output slots (include/spfm.h).
template <int M>
__global__ __launch_bounds__(kBlock) void obj_finish_kernel(const double* __restrict__ rec,
                                                            int nblk, int k, int reg,
                                                            int all_subsets, int is_w,
                                                            double* __restrict__ fin,
                                                            double* __restrict__ out8) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per = (nblk + kWave - 1) / kWave;
    for (int s = wave; s <= k; s += kBlock / kWave) {
        ObjPart<M> a;
        obj_init<M>(a);
        const int lo = lane * per, hi = (lo + per < nblk) ? lo + per : nblk;
        for (int c = lo; c < hi; ++c) {
            ObjPart<M> b;
            obj_load<M>(b, rec + ((size_t)c * (k + 1) + s) * kObjRec);
            obj_combine<M>(a, b);
        }
        obj_wave_reduce<M>(a);
        if (lane == 0) obj_store<M>(a, fin + (size_t)s * kObjRec);
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sumsq = 0.0, l1 = 0.0, sql12 = 0.0, ti = 0.0, nnz = 0.0, comps = 0.0;
    for (int s = 0; s < k; ++s) {
        const double* r = fin + (size_t)s * kObjRec;
        sumsq += r[OBJ_SUMSQ];
        l1 += r[OBJ_ABS];
        sql12 += r[OBJ_ABS] * r[OBJ_ABS];
        ti += all_subsets ? r[OBJ_PROD] : (M > 0 ? r[OBJ_E1 + (M > 0 ? M - 1 : 0)] : 0.0);
        nnz += r[OBJ_NNZ];
        comps += (r[OBJ_NNZ] > 0.0) ? 1.0 : 0.0;
    }
    const double* rn = fin + (size_t)k * kObjRec;
    double omega = 0.0;
    switch (reg) {
        case REG_L1: omega = l1; break;
        case REG_L21: omega = rn[OBJ_ABS]; break;
        case REG_SQL12: omega = sql12; break;
        case REG_SQL21: omega = rn[OBJ_ABS] * rn[OBJ_ABS]; break;
        case REG_OMEGATI: omega = ti; break;
        case REG_OMEGACS:
            omega = all_subsets ? rn[OBJ_PROD] : (M > 0 ? rn[OBJ_E1 + (M > 0 ? M - 1 : 0)] : 0.0);
            break;
    }
    out8[0] = 0.5 * sumsq;
    out8[1] = is_w ? 0.0 : omega;
    out8[2] = nnz;
    out8[3] = is_w ? 0.0 : rn[OBJ_NNZ];
    out8[4] = is_w ? 0.0 : comps;
    out8[5] = out8[6] = out8[7] = 0.0;
}

// per-block partial sums of loss(pred_i, y_i) over f64 vectors; finished by reduce_sum_kernel
static __global__ __launch_bounds__(kBlock) void eval_loss_partial_kernel(
    int64_t n, const double* __restrict__ pred, const double* __restrict__ y, int loss,
    double* __restrict__ partial) {
    __shared__ double red[16];
    double a = 0.0, b = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kBlock)
        a += loss_dev(loss, pred[i], y[i]);
    block_sum2(a, b, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
}

}  // namespace spfm
