// spfm_interactions3.hip.h -- third-order interaction weights of one parameter block:
//   T[a, j, l] = sum_s lams_s p_sa p_sj p_sl   over triples a < j < l,
// consumed in registers (spfm_interaction3_*, include/spfm.h).  Part of the gfx950 device code of
// the sparse-FM proximal CD core; see DESIGN.md section 14a.
//
// Built on the pair pass (spfm_interactions.hip.h): the same compaction, the same packed images
// A[jj][s] = p_{s, ids[jj]} and B = diag(lams) A, the same 64 x 64 tiles, LDS row stride, MFMA
// operand map, record reduction and radix select.  For a fixed smallest member a ("pivot"),
// T[a, :, :] is the pair product with the second operand scaled by p_{.a}:
//   T[a, j, l] = sum_s A[j][s] * (B[l][s] * A[a][s])
// and that is the definition in every mode, launch partition and tile budget: the scaling is one
// f64 multiply per fragment element (never fused), the sum the same chain of MFMA steps over
// s = 0, 4, 8, ... as int_tile_kernel.  All ids below are compacted ids; compaction is monotone,
// so a < j < l holds for the feature ids as well.
//
// int3_tile_kernel<MODE>: workgroup u of a launch owns unit unit0 + u = (pair tile (tj <= tl),
// pivot block ta <= tj): the 64 pivots of tile ta (those below the last row of tile tj when
// ta == tj).  Units are numbered tj-major, then ta, then tl, so neighbours share the A tile and
// the pivots.  The workgroup walks its pivots in ascending order; with one component chunk
// (k <= 32) the two operand tiles are staged through LDS once and stay there for all pivots,
// with more chunks they are restaged per pivot and chunk (the accumulators of ONE pivot live in
// registers, those of 64 would not).  The epilogues are the pair kernel's, with the mask
// a < j < l (a diagonal pair tile, a pivot inside tile tj and all three in one tile included):
//   INT_STATS  one record per unit, accumulated per thread over the unit's pivots in order, then
//              registers -> lanes -> waves as int_rec_block_reduce; int_reduce_kernel folds the
//              records.  The record count grows with pair tiles x pivot blocks, not with triples.
//   INT_HIST   as the pair pass, on the pattern of |T|
//   INT_EMIT   key = a << 42 | j << 21 | l in COMPACTED ids (kInt3IdBits = 21 bits each: the work
//              guard SPFM_INTERACTION3_MAX_ACTIVE keeps d_a far below 2^21, checked at compile
//              time; feature ids themselves may exceed 2^21 and are looked up through ids[] when
//              the host unpacks a key) and the value
// int3_values_kernel: T at L given triples, one thread each, straight from the live image.
#pragma once
#include "spfm_interactions.hip.h"

// SPFM_INTERACTION3_MAX_ACTIVE (include/spfm.h, documented there): the work guard of the triple
// passes, d_a^3 k / 3 flops each.
#include "../../include/spfm.h"

namespace spfm {

constexpr int kInt3IdBits = 21;                    // bits per compacted id in an emitted key
constexpr long long kInt3Window = 1ll << 18;       // units whose records exist at a time (x kIntRun)
static_assert(SPFM_INTERACTION3_MAX_ACTIVE + kIntTile <= (1 << kInt3IdBits),
              "three compacted ids must fit a 64-bit key");
static_assert(kInt3Window % kIntRun == 0, "a window is whole runs");

struct Int3Args {
    IntArgs p;  // as the pair pass; p.tile0 = first unit of this launch, p.rec_base in units
    int da;     // active features: pivots stop here
};

// units (tj', ta, tl) with tj' < tj:  sum_{t < tj} (t + 1) (T - t)
__host__ __device__ __forceinline__ long long int3_units_before(long long tj, long long T) {
    return T * (tj * (tj + 1) / 2) - (tj - 1) * tj * (tj + 1) / 3;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void int3_tile_kernel(Int3Args a3) {
    __shared__ double sA[kIntTile * kIntLd];
    __shared__ double sB[kIntTile * kIntLd];
    __shared__ unsigned sHist[MODE == INT_HIST ? kIntHistBins : 1];
    __shared__ IntRec red[kBlock / kWave];
    const IntArgs& a = a3.p;

    // unit number -> (tj, ta <= tj, tl >= tj): tj by bisection on the exact integer count
    const long long u = a.tile0 + blockIdx.x, T = a.T;
    long long lo = 0, hi = T - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (int3_units_before(mid, T) <= u) lo = mid; else hi = mid - 1;
    }
    const long long tj = lo, rem = u - int3_units_before(tj, T);
    const long long ta = rem / (T - tj), tl = tj + rem % (T - tj);
    // pivots of tile ta; a < j leaves out the last row of tile tj
    const long long p0 = ta * kIntTile;
    long long p1 = (ta == tj) ? p0 + kIntTile - 1 : p0 + kIntTile;
    if (p1 > a3.da) p1 = a3.da;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;

    int_hist_clear<MODE>(sHist);
    IntRec mine;
    mine.cnt = 0;
    mine.sumsq = mine.sumabs = mine.maxabs = 0.0;

    const double* Ag = a.A + (size_t)tj * kIntTile * a.kp;
    const double* Bg = a.B + (size_t)tl * kIntTile * a.kp;
    const bool restage = a.kp > kIntKC;  // more than one chunk: the tiles cannot stay in LDS
    // kp is k >= 1 padded to a multiple of 4: every pivot has a chunk.  Said here so that the
    // accumulators go from the last MFMA straight into the epilogue, with no second way in
    __builtin_assume(a.kp > 0);
    for (long long piv = p0; piv < p1; ++piv) {
        int_v4d acc[2][2];
        int_acc_zero(acc);
        const double* pp = a.A + (size_t)piv * a.kp + l4;  // the lane's components of the pivot
        for (int kc0 = 0; kc0 < a.kp; kc0 += kIntKC) {
            const int kend = (a.kp - kc0 < kIntKC) ? a.kp - kc0 : kIntKC;  // multiple of 4
            if (restage || piv == p0)  // workgroup-uniform
                int_stage_chunk(Ag, Bg, a.kp, kc0, kend, sA, sB);
            int_mfma_chunk<true>(sA, sB, kend, pp + kc0, acc);
        }

        // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long gj = tj * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
                    const long long gl = tl * kIntTile + wc * 32 + cb * 16 + l15;
                    const double w = acc[ra][cb][r];
                    const double m = (piv < gj && gj < gl) ? fabs(w) : 0.0;  // a < j < l only
                    int_consume<MODE>(
                        a, w, m,
                        [&] {
                            return ((unsigned long long)piv << (2 * kInt3IdBits)) |
                                   ((unsigned long long)gj << kInt3IdBits) | (unsigned long long)gl;
                        },
                        mine, sHist);
                }
    }
    int_finish<MODE>(a, u, mine, red, sHist);
}

// T at L triples: one thread per triple, the three ids in any order (sorted here, the smallest is
// the pivot), components in order s = 0..k-1; any two equal ids give 0
static __global__ __launch_bounds__(kBlock) void int3_values_kernel(
    const double* __restrict__ base, int64_t ss, int64_t sj, int k, const double* __restrict__ lams,
    long long L, const int32_t* __restrict__ i0, const int32_t* __restrict__ i1,
    const int32_t* __restrict__ i2, double* __restrict__ out) {
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (q >= L) return;
    int64_t x = i0[q], y = i1[q], z = i2[q], t;
    if (x > y) { t = x; x = y; y = t; }
    if (y > z) { t = y; y = z; z = t; }
    if (x > y) { t = x; x = y; y = t; }
    double acc = 0.0;
    if (x != y && y != z)
        for (int s = 0; s < k; ++s)
            acc += base[s * ss + y * sj] * ((lams[s] * base[s * ss + z * sj]) * base[s * ss + x * sj]);
    out[q] = acc;
}

}  // namespace spfm
