// spfm_interactions.hip.h -- selected feature interactions of one parameter block:
// W = P_o^T diag(lams) P_o over pairs j < j', consumed in registers (spfm_interaction_*,
// include/spfm.h).  Part of the gfx950 device code of the sparse-FM proximal CD core; see
// DESIGN.md section 14.
//
// The block is read through element strides like obj_block_kernel (spfm_objective.hip.h): element
// (s, j) lives at base[s * ss + j * sj], whichever of the (k,d) / (d,k) images is live.
//
// 1. Compaction.  int_flag_kernel marks the features with any non-zero entry, a prefix scan gives
//    every active feature its rank, int_pack_kernel writes two packed images of the d_a active
//    columns, feature-major with k padded to a multiple of 4 and d_a to a multiple of 64 (zeros):
//    A[jj][s] = p_{s, ids[jj]} and B[jj][s] = lams[s] * A[jj][s] (lams is +-1: exact).
// 2. int_tile_kernel<MODE>: workgroup t of a launch owns the 64 x 64 tile (ti <= tj) number
//    tile0 + t of the upper triangle of the d_a x d_a product, in row-major tile order.  The
//    operands are staged through LDS in chunks of 32 components; the four waves form a 2 x 2 grid
//    of 32 x 32 quadrants, each four v_mfma_f64_16x16x4_f64 accumulators (16 doubles per lane).
//    Every value of W is the same chain of MFMA steps over s = 0, 4, 8, ... whatever the mode, the
//    launch partition or the tile budget: all modes see the same bits.  W is never stored; the
//    epilogue of the mode consumes the accumulators:
//      INT_STATS  one record per tile (count of |W| > tol, sum W^2, sum |W|, max |W|), reduced in
//                 a fixed order: registers, lanes (shuffle tree), waves in order
//      INT_HIST   histogram of bits [bin_shift, bin_shift + bits) of the f64 pattern of |W| over
//                 the W != 0 whose higher bits equal `prefix` (LDS counts per tile, then integer
//                 atomics: exact, order-free)
//      INT_EMIT   every pair with |W| > tol and pattern >= thr_key appended (wave-aggregated
//                 ticket) as key = row id << 32 | column id and value; the ticket counts ALL such
//                 pairs, entries beyond `cap` are dropped
//    A diagonal tile keeps j < j' only.
// 3. int_reduce_kernel: records -> one record per run of 4096 records (thread t the records
//    t, t + 256, ... of the run in order, lanes, waves in order); applied until one is left.  Tile
//    records exist for one window of 2^22 tiles at a time and are folded into their runs before
//    the next window starts, so that only the run records grow with the tile count.  The tree
//    depends on the tile count alone.
#pragma once
#include "spfm_common.hip.h"

namespace spfm {

constexpr int kIntTile = 64;             // features per tile side
constexpr int kIntKC = 32;               // components per LDS chunk
constexpr int kIntLd = kIntKC + 4;       // LDS row stride (doubles): 2-way conflicts at most
constexpr int kIntRun = 4096;            // records per workgroup of the reduction
constexpr long long kIntWindow = 1ll << 22;  // tiles whose records exist at a time (x kIntRun)
constexpr int kIntHistBins = 4096;
enum { INT_STATS = 0, INT_HIST = 1, INT_EMIT = 2 };

struct IntRec {
    long long cnt;
    double sumsq, sumabs, maxabs;
};

struct IntArgs {
    const double* A;   // (d_a padded, kp)
    const double* B;
    const int32_t* ids;  // compact index -> feature id
    int kp, T;           // padded components; tiles per side
    long long tile0;     // first tile of this launch
    double tol;
    IntRec* rec;                      // INT_STATS record of tile t at rec[t - rec_base]
    long long rec_base;
    unsigned long long* hist;         // INT_HIST  [kIntHistBins]
    unsigned long long prefix;        // INT_HIST  high bits that must match (prefix_shift < 64)
    int prefix_shift, bin_shift;
    unsigned bin_mask;
    unsigned long long thr_key;       // INT_EMIT
    unsigned long long cap;
    unsigned long long* counter;
    unsigned long long* keys;
    double* vals;
};

typedef double int_v4d __attribute__((ext_vector_type(4)));

static __global__ __launch_bounds__(kBlock) void int_flag_kernel(const double* __restrict__ base,
                                                                 int64_t ss, int64_t sj, int k,
                                                                 int d, int dlim,
                                                                 int32_t* __restrict__ flag) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= d) return;
    int any = 0;
    if (j < dlim)
        for (int s = 0; s < k; ++s) any |= (base[s * ss + j * sj] != 0.0) ? 1 : 0;
    flag[j] = any;
}

// ids[rank] = j for the active features; total[0] = d_a
static __global__ __launch_bounds__(kBlock) void int_compact_kernel(
    const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int d,
    int32_t* __restrict__ ids, int32_t* __restrict__ total) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= d) return;
    if (flag[j]) ids[pos[j]] = j;
    if (j == d - 1) total[0] = pos[j] + flag[j];
}

// one thread per element of the padded images
static __global__ __launch_bounds__(kBlock) void int_pack_kernel(
    const double* __restrict__ base, int64_t ss, int64_t sj, int k, int kp, int da, int64_t total,
    const int32_t* __restrict__ ids, const double* __restrict__ lams, double* __restrict__ A,
    double* __restrict__ B) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const int64_t jj = e / kp;
    const int s = (int)(e - jj * kp);
    double p = 0.0, l = 0.0;
    if (jj < da && s < k) {
        p = base[s * ss + (int64_t)ids[jj] * sj];
        l = lams[s];
    }
    A[e] = p;
    B[e] = l * p;
}

__device__ __forceinline__ void int_rec_combine(IntRec& a, const IntRec& b) {
    a.cnt += b.cnt;
    a.sumsq += b.sumsq;
    a.sumabs += b.sumabs;
    a.maxabs = fmax(a.maxabs, b.maxabs);
}

// lane 0 of every wave ends up with the wave's record (fixed shuffle tree), thread 0 with the
// workgroup's (waves in order)
__device__ __forceinline__ void int_rec_block_reduce(IntRec& a, IntRec* red /*[4]*/) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        IntRec b;
        b.cnt = __shfl_down(a.cnt, off, kWave);
        b.sumsq = __shfl_down(a.sumsq, off, kWave);
        b.sumabs = __shfl_down(a.sumabs, off, kWave);
        b.maxabs = __shfl_down(a.maxabs, off, kWave);
        int_rec_combine(a, b);  // lanes without a partner combine garbage; lane 0 never does
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / kWave; ++w) int_rec_combine(a, red[w]);
}

// ---- the pieces int_tile_kernel and int3_tile_kernel (spfm_interactions3.hip.h) are made of ----

// Chunk staging: components [kc0, kc0 + kend) of the 64 rows at Ag / Bg -> sA / sB (row stride
// kIntLd, zeros up to kIntKC), between two barriers
__device__ __forceinline__ void int_stage_chunk(const double* __restrict__ Ag,
                                                const double* __restrict__ Bg, int kp, int kc0,
                                                int kend, double* sA, double* sB) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kIntTile * kIntKC / kBlock; ++i) {
        const int idx = tid + i * kBlock, r = idx / kIntKC, c = idx % kIntKC;
        const bool in = c < kend;
        sA[r * kIntLd + c] = in ? Ag[(size_t)r * kp + kc0 + c] : 0.0;
        sB[r * kIntLd + c] = in ? Bg[(size_t)r * kp + kc0 + c] : 0.0;
    }
    __syncthreads();
}

__device__ __forceinline__ void int_acc_zero(int_v4d (&acc)[2][2]) {
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) acc[ra][cb] = (int_v4d){0.0, 0.0, 0.0, 0.0};
}

// MFMA chunk step: the staged chunk into the wave's 32 x 32 quadrant (wave = 2 * wr + wc), four
// accumulators.  Operand maps of v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4]
// and B[k = l >> 4][col l & 15].  PIVOT: the B fragment is scaled by pp[kk], the lane's component
// of the pivot (one f64 multiply per fragment element); the pair form has no multiply.
template <bool PIVOT>
__device__ __forceinline__ void int_mfma_chunk(const double* sA, const double* sB, int kend,
                                               const double* __restrict__ pp,
                                               int_v4d (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
    const double* pa = sA + (wr * 32 + l15) * kIntLd + l4;
    const double* pb = sB + (wc * 32 + l15) * kIntLd + l4;
    for (int kk = 0; kk < kend; kk += 4) {
        const double a0 = pa[kk], a1 = pa[16 * kIntLd + kk];
        double b0 = pb[kk], b1 = pb[16 * kIntLd + kk];
        if constexpr (PIVOT) {
            const double ps = pp[kk];
            b0 *= ps;
            b1 *= ps;
        }
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}

// One 64 x 64 tile of the pair form: the rows at Ag against the rows at Bg over kp components,
// into the wave's quadrant
__device__ __forceinline__ void int_tile_product(const double* Ag, const double* Bg, int kp,
                                                 double* sA, double* sB, int_v4d (&acc)[2][2]) {
    int_acc_zero(acc);
    for (int kc0 = 0; kc0 < kp; kc0 += kIntKC) {
        const int kend = (kp - kc0 < kIntKC) ? kp - kc0 : kIntKC;  // multiple of 4
        int_stage_chunk(Ag, Bg, kp, kc0, kend, sA, sB);
        int_mfma_chunk<false>(sA, sB, kend, nullptr, acc);
    }
}

// LDS of the two staging tiles
static inline size_t int_stage_lds_bytes() { return sizeof(double) * 2 * kIntTile * kIntLd; }

template <int MODE>
__device__ __forceinline__ void int_hist_clear(unsigned* sHist) {
    if constexpr (MODE == INT_HIST) {
        for (int b = threadIdx.x; b < kIntHistBins; b += kBlock) sHist[b] = 0u;
    }
}

// Per-value epilogue: the value w, its magnitude m (0 where the kernel's mask leaves the value
// out) and key(), the key to emit (called for the values that are stored only).  Wave-uniform
// control flow: every lane of the wave calls it for every value.
template <int MODE, typename KeyFn>
__device__ __forceinline__ void int_consume(const IntArgs& a, double w, double m, KeyFn key,
                                            IntRec& mine, unsigned* sHist) {
    if constexpr (MODE == INT_STATS) {
        mine.cnt += (m > a.tol) ? 1 : 0;
        mine.sumsq += m * m;
        mine.sumabs += m;
        mine.maxabs = fmax(mine.maxabs, m);
    } else if constexpr (MODE == INT_HIST) {
        const unsigned long long pat = (unsigned long long)__double_as_longlong(m);
        if (m > 0.0 && (a.prefix_shift >= 64 || (pat >> a.prefix_shift) == a.prefix))
            atomicAdd(&sHist[(unsigned)(pat >> a.bin_shift) & a.bin_mask], 1u);
    } else {
        const int lane = threadIdx.x & 63;
        const unsigned long long pat = (unsigned long long)__double_as_longlong(m);
        const bool take = m > a.tol && pat >= a.thr_key;
        const unsigned long long mask = __ballot(take);
        if (mask != 0ull) {  // wave-uniform
            const int leader = __ffsll((long long)mask) - 1;
            unsigned long long slot = 0ull;
            if (lane == leader) slot = atomicAdd(a.counter, (unsigned long long)__popcll(mask));
            slot = __shfl(slot, leader, kWave);
            if (take) {
                slot += (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                if (slot < a.cap) {
                    a.keys[slot] = key();
                    a.vals[slot] = w;
                }
            }
        }
    }
}

// Closing step of workgroup `unit`: its record (lanes, then waves in order), or its histogram
template <int MODE>
__device__ __forceinline__ void int_finish(const IntArgs& a, long long unit, IntRec& mine,
                                           IntRec* red, const unsigned* sHist) {
    if constexpr (MODE == INT_STATS) {
        int_rec_block_reduce(mine, red);
        if (threadIdx.x == 0) a.rec[unit - a.rec_base] = mine;
    } else if constexpr (MODE == INT_HIST) {
        __syncthreads();
        for (int b = threadIdx.x; b < kIntHistBins; b += kBlock) {
            const unsigned c = sHist[b];
            if (c) atomicAdd(&a.hist[b], (unsigned long long)c);
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void int_tile_kernel(IntArgs a) {
    __shared__ double sA[kIntTile * kIntLd];
    __shared__ double sB[kIntTile * kIntLd];
    __shared__ unsigned sHist[MODE == INT_HIST ? kIntHistBins : 1];
    __shared__ IntRec red[kBlock / kWave];

    // tile number -> (ti <= tj), row-major over the upper triangle
    const long long t = a.tile0 + blockIdx.x, T = a.T;
    const double tw = 2.0 * (double)T + 1.0;
    long long ti = (long long)((tw - sqrt(tw * tw - 8.0 * (double)t)) * 0.5);
    if (ti < 0) ti = 0;
    if (ti > T - 1) ti = T - 1;
    while (ti + 1 < T && (ti + 1) * T - (ti + 1) * ti / 2 <= t) ++ti;
    while (ti > 0 && ti * T - ti * (ti - 1) / 2 > t) --ti;
    const long long tj = ti + (t - (ti * T - ti * (ti - 1) / 2));

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;

    int_hist_clear<MODE>(sHist);
    int_v4d acc[2][2];
    int_tile_product(a.A + (size_t)ti * kIntTile * a.kp, a.B + (size_t)tj * kIntTile * a.kp, a.kp,
                     sA, sB, acc);

    // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15
    IntRec mine;
    mine.cnt = 0;
    mine.sumsq = mine.sumabs = mine.maxabs = 0.0;
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long gi = ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
                const long long gj = tj * kIntTile + wc * 32 + cb * 16 + l15;
                const double w = acc[ra][cb][r];
                const double m = (gi < gj) ? fabs(w) : 0.0;  // diagonal tile: j < j' only
                int_consume<MODE>(
                    a, w, m,
                    [&] {
                        return ((unsigned long long)(unsigned)a.ids[gi] << 32) |
                               (unsigned long long)(unsigned)a.ids[gj];
                    },
                    mine, sHist);
            }
    int_finish<MODE>(a, t, mine, red, sHist);
}

// out[b] = the records [b * kIntRun, min(n, (b + 1) * kIntRun)) combined in a fixed order
static __global__ __launch_bounds__(kBlock) void int_reduce_kernel(const IntRec* __restrict__ in,
                                                                   long long n,
                                                                   IntRec* __restrict__ out) {
    __shared__ IntRec red[kBlock / kWave];
    const long long lo = (long long)blockIdx.x * kIntRun;
    const long long hi = (lo + kIntRun < n) ? lo + kIntRun : n;
    IntRec a;
    a.cnt = 0;
    a.sumsq = a.sumabs = a.maxabs = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += kBlock) int_rec_combine(a, in[i]);
    int_rec_block_reduce(a, red);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// W at L pairs: one thread per pair, components in order; j == j' gives 0 (no diagonal)
static __global__ __launch_bounds__(kBlock) void int_values_kernel(
    const double* __restrict__ base, int64_t ss, int64_t sj, int k, const double* __restrict__ lams,
    long long L, const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
    double* __restrict__ out) {
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (q >= L) return;
    const int64_t j = rows[q], j2 = cols[q];
    double acc = 0.0;
    if (j != j2)
        for (int s = 0; s < k; ++s) acc += (lams[s] * base[s * ss + j * sj]) * base[s * ss + j2 * sj];
    out[q] = acc;
}

// the dense sub-block W[J, J2] (row-major nJ x nJ2), same arithmetic as int_values_kernel
static __global__ __launch_bounds__(kBlock) void int_block_kernel(
    const double* __restrict__ base, int64_t ss, int64_t sj, int k, const double* __restrict__ lams,
    long long nJ, const int32_t* __restrict__ J, long long nJ2, const int32_t* __restrict__ J2,
    double* __restrict__ out) {
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (q >= nJ * nJ2) return;
    const int64_t j = J[q / nJ2], j2 = J2[q % nJ2];
    double acc = 0.0;
    if (j != j2)
        for (int s = 0; s < k; ++s) acc += (lams[s] * base[s * ss + j * sj]) * base[s * ss + j2 * sj];
    out[q] = acc;
}

}  // namespace spfm
