// spfm_rankeval.hip.h -- exact ranks of held-out candidates (spfm_rank_eval, include/spfm.h).
// Part of the gfx950 device code of the sparse-FM proximal CD core; see DESIGN.md section 15a.
//
// Per context row b a list of targets T_b and a list of excluded candidates E_b (CSR patterns,
// ascending, disjoint).  rank[b, t] = the number of candidates c outside E_b, c != t, whose
// (score, id) beats (score[b, t], t) under rank_beats.  Two kernels, both consumers of the 64 x 64
// score tiles of rank_tile_kernel (spfm_rank.hip.h): the same int_tile_product and the same
// closing + (rowconst + colconst), hence the same bits for every pair.
//
// 1. rank_tscore_kernel: one workgroup per (row tile, candidate tile) pair that holds a target
//    (a work list the host makes from the patterns).  Wave 0, lane = row, finds by binary search
//    where the tile's columns start in the row's target list and turns the targets in the tile
//    into a 64-bit mask; the epilogue stores a score whose bit is set at the target's position
//    (list start + the number of mask bits below its own).
// 2. rank_count_kernel<EXCL>: workgroup (strip, row tile) like the selection.  In LDS per row:
//    its targets sorted by rank_beats with their (score, id) (one wave per row, one lane per
//    target, positions by counting over lane broadcasts), a permutation back to the list order and
//    tcap + 1 integer buckets.  The (score, id) of each row's weakest target stays in registers:
//    an admissible in-range finite score that does not beat it is dropped after that one compare.
//    Otherwise a binary search gives the first sorted target it beats -- it beats all later ones
//    -- and one integer LDS atomic counts it there.  A target meets itself as a candidate and
//    lands one past its own position.  At the end of the strip a wave per row forms the inclusive
//    prefix sums of the buckets, the per-target counts of the strip, and adds them into the
//    call's int32 array with integer atomics (they commute: no result depends on the strips).
//    The exclusion masks are RankExcl's (spfm_rank.hip.h).
//    A target whose score is not finite is sorted as -inf and gets rank -1 on the host; a
//    candidate whose score is not finite is never counted.
// No float atomics, no waiting between workgroups.
#pragma once
#include "spfm_rank.hip.h"

namespace spfm {

constexpr int kRankMaxTargets = 64;  // SPFM_RANK_MAX_TARGETS: one lane per target of a row
static_assert(kRankMaxTargets <= kWave && kRankMaxTargets <= 255, "lane per target, uint8 perm");

struct RankEvalArgs {
    RankArgs r;           // towers, constants, partition, exclusion lists
    const int64_t* tptr;  // targets of every context row of the call (CSR pattern, ascending)
    const int32_t* tidx;
    const int2* pairs;    // rank_tscore_kernel: (row tile of the slab, candidate tile)
    double* tscore;       // aligned with tidx
    int32_t* trank;       // aligned with tidx; cleared by the caller, accumulated over the strips
    int tcap;             // the largest number of targets of a row of the call, >= 1
};

// dynamic LDS of rank_count_kernel
static inline size_t rank_count_lds_bytes(int tcap) {
    return int_stage_lds_bytes() +
           (size_t)kIntTile * tcap * (sizeof(double) + sizeof(int32_t) + sizeof(uint8_t)) +
           (size_t)kIntTile * (tcap + 1) * sizeof(int) +
           kIntTile * (sizeof(unsigned long long) + sizeof(int));
}

static __global__ __launch_bounds__(kBlock) void rank_tscore_kernel(RankEvalArgs e) {
    __shared__ double sA[kIntTile * kIntLd];
    __shared__ double sB[kIntTile * kIntLd];
    __shared__ unsigned long long tmask[kIntTile];
    __shared__ int64_t tstart[kIntTile];
    const RankArgs& a = e.r;
    const int ti = e.pairs[blockIdx.x].x, tj = e.pairs[blockIdx.x].y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;

    if (wave == 0) {
        unsigned long long m = 0ull;
        int64_t cur = 0;
        if (ti * kIntTile + lane < a.nrow) {
            const int64_t row = a.row0 + ti * kIntTile + lane, end = e.tptr[row + 1];
            cur = rank_lower_bound(e.tidx, e.tptr[row], end, tj * kIntTile);
            int64_t c = cur;
            m = rank_mask_step(e.tidx, c, end, tj * kIntTile);
        }
        tmask[lane] = m;
        tstart[lane] = cur;
        // (published by the barriers of the staging step)
    }
    double rcv[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            rcv[ra][r] = a.rc[(size_t)ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r];

    int_v4d acc[2][2];
    int_tile_product(a.U + (size_t)ti * kIntTile * a.Rp, a.V + (size_t)tj * kIntTile * a.Rp, a.Rp,
                     sA, sB, acc);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int bit = wc * 32 + cb * 16 + l15;
        const double ccv = a.cc[tj * kIntTile + bit];  // padded to whole tiles
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = wr * 32 + ra * 16 + l4 + 4 * r;
                const double v = acc[ra][cb][r] + (rcv[ra][r] + ccv);
                const unsigned long long m = tmask[rl];
                // a set bit: the row exists and the column is one of its targets (< C)
                if ((m >> bit) & 1ull)
                    e.tscore[tstart[rl] + __popcll(m & ((1ull << bit) - 1ull))] = v;
            }
    }
}

template <bool EXCL>
__global__ __launch_bounds__(kBlock) void rank_count_kernel(RankEvalArgs e) {
    extern __shared__ double rank_count_lds[];
    const RankArgs& a = e.r;
    const int tcap = e.tcap, hld = tcap + 1;
    double* sA = rank_count_lds;
    double* sB = sA + kIntTile * kIntLd;
    double* tv = sB + kIntTile * kIntLd;                                         // [64][tcap]
    [[maybe_unused]] RankExcl ex{reinterpret_cast<unsigned long long*>(tv + (size_t)kIntTile * tcap)};
    int32_t* tc = reinterpret_cast<int32_t*>(ex.mask + kIntTile);                // [64][tcap]
    int* hist = tc + (size_t)kIntTile * tcap;                                    // [64][tcap + 1]
    int* ntg = hist + (size_t)kIntTile * hld;                                    // [64]
    uint8_t* perm = reinterpret_cast<uint8_t*>(ntg + kIntTile);                  // [64][tcap]

    const int strip = blockIdx.x, ti = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int Tc = (a.C + kIntTile - 1) / kIntTile;
    const int t0 = strip * a.strip_tiles;
    const int t1 = (t0 + a.strip_tiles < Tc) ? t0 + a.strip_tiles : Tc;

    // the targets of every row, sorted: (score descending, id ascending)
    for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
        int n = 0;
        int64_t b = 0;
        if (ti * kIntTile + rl < a.nrow) {
            b = e.tptr[a.row0 + ti * kIntTile + rl];
            n = (int)(e.tptr[a.row0 + ti * kIntTile + rl + 1] - b);
        }
        n = __builtin_amdgcn_readfirstlane(n);  // wave-uniform
        double v = 0.0;
        int c = 0;
        if (lane < n) {
            v = e.tscore[b + lane];
            c = e.tidx[b + lane];
            if (!(fabs(v) < INFINITY)) v = -INFINITY;  // rank -1 in the end; keeps the order total
        }
        int p = 0;
        for (int l = 0; l < n; ++l) {
            const double vj = readlane_d(v, l);
            const int cj = __builtin_amdgcn_readlane(c, l);
            p += rank_beats(vj, (unsigned)cj, v, (unsigned)c) ? 1 : 0;
        }
        if (lane < n) {
            tv[rl * tcap + p] = v;
            tc[rl * tcap + p] = c;
            perm[rl * tcap + p] = (uint8_t)lane;
        }
        for (int q = lane; q < hld; q += kWave) hist[rl * hld + q] = 0;
        if (lane == 0) ntg[rl] = n;
    }
    __syncthreads();

    // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15.
    // The weakest target of the lane's eight rows; a row without targets: nothing beats (+inf, 0)
    double rcv[2][4], wkv[2][4];
    unsigned wkc[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = wr * 32 + ra * 16 + l4 + 4 * r;
            rcv[ra][r] = a.rc[(size_t)ti * kIntTile + rl];
            const int n = ntg[rl];
            wkv[ra][r] = n ? tv[rl * tcap + n - 1] : INFINITY;
            wkc[ra][r] = n ? (unsigned)tc[rl * tcap + n - 1] : 0u;
        }

    if constexpr (EXCL) ex.open(a, ti, t0 * kIntTile);

    const double* Ug = a.U + (size_t)ti * kIntTile * a.Rp;
    for (int tj = t0; tj < t1; ++tj) {
        if constexpr (EXCL) ex.tile(a, tj);
        int_v4d acc[2][2];
        int_tile_product(Ug, a.V + (size_t)tj * kIntTile * a.Rp, a.Rp, sA, sB, acc);
        [[maybe_unused]] unsigned long long em[2][4];
        if constexpr (EXCL) ex.rows(em);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int bit = wc * 32 + cb * 16 + l15;
            const int col = tj * kIntTile + bit;
            const double ccv = a.cc[col];  // padded to whole tiles
#pragma unroll
            for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[ra][cb][r] + (rcv[ra][r] + ccv);
                    bool in = col < a.C && fabs(v) < INFINITY;
                    if constexpr (EXCL) in = in && !((em[ra][r] >> bit) & 1ull);
                    if (in && rank_beats(v, (unsigned)col, wkv[ra][r], wkc[ra][r])) {
                        const int rl = wr * 32 + ra * 16 + l4 + 4 * r;
                        const double* rv = tv + rl * tcap;
                        const int32_t* rcd = tc + rl * tcap;
                        int lo = 0, hi = ntg[rl] - 1;  // the first target (v, col) beats
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (rank_beats(v, (unsigned)col, rv[mid], (unsigned)rcd[mid]))
                                hi = mid;
                            else
                                lo = mid + 1;
                        }
                        atomicAdd(&hist[rl * hld + lo], 1);
                    }
                }
        }
    }
    __syncthreads();
    for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
        const int n = __builtin_amdgcn_readfirstlane(ntg[rl]);
        if (n == 0) continue;  // wave-uniform
        int h = lane < n ? hist[rl * hld + lane] : 0;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int t = __shfl_up(h, off, kWave);
            if (lane >= off) h += t;
        }
        if (lane < n && h != 0)
            atomicAdd(&e.trank[e.tptr[a.row0 + ti * kIntTile + rl] + perm[rl * tcap + lane]], h);
    }
}

}  // namespace spfm
