// spfm_rank.hip.h -- candidate ranking: scores of every (context row, candidate row) pair of a
// fitted model and the K best candidates per context (spfm_rank_*, include/spfm.h).  Part of the
// gfx950 device code of the sparse-FM proximal CD core; see DESIGN.md section 15.
//
// For rows x, z with disjoint supports the ANOVA kernel splits,
//   a_s^m(x + z) = sum_{t=0..m} a_s^t(x) a_s^{m-t}(z),
// and so does the all-subsets product, hence
//   score[b, c] = rowconst[b] + colconst[c] + sum_r U[b, r] V[c, r]
// with R = k (m - 1) columns per ANOVA block of degree m and k for the all-subsets block.
//
// 1. tower_kernel<T, M>: one wavefront per row, lanes over components, the DP a[0..M] in
//    registers (anova_predict_kernel's recurrence).  The context side writes lams_s a_s^t(x) into
//    column col0 + (t - 1) k + s (lams is +-1: exact) and adds w.x + sum_s lams_s a_s^M(x) to the
//    row's constant; the candidate side writes a_s^{M-t}(z) into the same column and adds the same
//    constant of z.  M = 0 (all-subsets): the one column s holds lams_s prod (1 + p x) / prod
//    (1 + p z) and there is no constant.  Images are row-major, R padded to a multiple of 4 and
//    rows to a multiple of 64, with zeros (the caller clears them first).
// 2. rank_tile_kernel<MODE>: workgroup (strip, ti) owns the 64-row context tile ti against the
//    candidate tiles of its strip, one after the other.  The tile product is int_tile_product
//    (spfm_interactions.hip.h); a score is acc + (rowconst + colconst), the same bits in every
//    mode and under every slab / strip partition.
//      RANK_DENSE   stores the tile
//      RANK_SELECT  the streaming top-K selection of spfm_select.hip.h on the scores themselves
//                   (floor -inf): per strip a sorted list of every context row's K best.
//                   Non-finite scores never enter a list.
//    rank_merge_kernel: sel_merge of the per-strip lists, one wave per context row.
//    EXCL (spfm_rank_topk_excl): per context row an ascending list of
//    candidates that are left out.  Before a tile is staged, wave 0 (lane = row of the tile)
//    turns each row's list into one 64-bit mask of the tile's columns (RankExcl: a cursor per
//    row, kept across the tiles of the strip, found by binary search where the strip starts); the
//    masks sit in LDS (512 B) and a score survives only if its bit is clear.  EXCL = false is the
//    code without any of this.
#pragma once
#include "spfm_select.hip.h"

namespace spfm {

constexpr int kRankMaxK = kSelMaxK;  // SPFM_RANK_MAX_K
enum { RANK_DENSE = 0, RANK_SELECT = 1 };
enum { RANK_CTX = 0, RANK_CAND = 1 };

struct RankArgs {
    const double* U;    // (rows padded, Rp) of the slab
    const double* V;    // (candidates padded, Rp)
    const double* rc;   // rowconst of the slab (padded)
    const double* cc;   // colconst (padded)
    int Rp, nrow, C;    // padded columns; context rows of the slab; candidates
    int strip_tiles, n_strips, rows_pad;
    double* dense;      // RANK_DENSE (nrow, C)
    SelLists sel;       // RANK_SELECT, rank_merge_kernel; K = min(K, C)
    const int64_t* eptr;  // EXCL: excluded candidates of every context row of the call (CSR
    const int32_t* eidx;  //       pattern, ascending per row), row `row0 + r` for slab row r
    int64_t row0;
};

// Dynamic LDS of rank_tile_kernel: the staging tiles (int_stage_lds_bytes), RANK_SELECT: + the
// selection (SelPlan::lds), EXCL: + the masks
constexpr size_t kRankExclLdsBytes = kIntTile * sizeof(unsigned long long);

template <typename T, int M>
__global__ __launch_bounds__(kBlock) void tower_kernel(
    int64_t row0, int64_t rows, int k, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ ridx, const T* __restrict__ rval, const double* __restrict__ base,
    int64_t ss, int64_t sj, const double* __restrict__ lams,
    const double* __restrict__ w /* NULL: no linear term */, int side, int Rp, int col0,
    double* __restrict__ img, double* __restrict__ cst /* accumulated */) {
    const int64_t local = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (local >= rows) return;
    const int64_t b = rptr[row0 + local], e = rptr[row0 + local + 1];
    double* out = img + (size_t)local * Rp + col0;
    double acc = 0.0;
    for (int s = lane; s < k; s += kWave) {
        const double lam = lams[s];
        const auto px = [&](int64_t ii) {
            return base[s * ss + (int64_t)ridx[ii] * sj] * (double)rval[ii];
        };
        if constexpr (M == 0) {
            double a = 1.0;
            subsets_dp_add(a, b, e, px);
            out[s] = (side == RANK_CTX) ? lam * a : a;
        } else {
            double a[M + 1];
            anova_dp_init<M>(a);
            anova_dp_add<M>(a, b, e, px);
#pragma unroll
            for (int t = 1; t < M; ++t)
                out[(size_t)(t - 1) * k + s] = (side == RANK_CTX) ? lam * a[t] : a[M - t];
            acc += a[M] * lam;
        }
    }
    if (w != nullptr)
        for (int64_t ii = b + lane; ii < e; ii += kWave) acc += (double)rval[ii] * w[ridx[ii]];
    acc = wave_sum(acc);
    if (lane == 0) cst[local] += acc;
}

// first position in [lo, hi) of the ascending list idx whose id is >= key
__device__ __forceinline__ int64_t rank_lower_bound(const int32_t* __restrict__ idx, int64_t lo,
                                                    int64_t hi, int key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (idx[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The ids of the ascending list idx[cur, end) that fall into the tile [col0, col0 + 64), as a
// mask; cur moves past them.  idx[cur] >= col0 on entry (the tiles are visited in ascending order)
__device__ __forceinline__ unsigned long long rank_mask_step(const int32_t* __restrict__ idx,
                                                             int64_t& cur, int64_t end, int col0) {
    unsigned long long m = 0ull;
    while (cur < end) {
        const int c = idx[cur] - col0;
        if (c >= kIntTile) break;
        m |= 1ull << c;
        ++cur;
    }
    return m;
}

// EXCL, in rank_tile_kernel and rank_count_kernel: the exclusion masks of a workgroup's 64 rows
struct RankExcl {
    unsigned long long* mask;   // LDS [64]: the columns of the current tile that the row leaves out
    int64_t cur = 0, end = 0;   // wave 0, lane = row of the tile: the row's cursor into eidx

    // the cursors at the strip's first candidate col0
    __device__ __forceinline__ void open(const RankArgs& a, int ti, int col0) {
        const int lane = threadIdx.x & 63;
        if (threadIdx.x < kWave && ti * kIntTile + lane < a.nrow) {
            const int64_t row = a.row0 + ti * kIntTile + lane;
            end = a.eptr[row + 1];
            cur = rank_lower_bound(a.eidx, a.eptr[row], end, col0);
        }
    }
    // before tile tj is staged: its masks (published by the barriers of the staging step)
    __device__ __forceinline__ void tile(const RankArgs& a, int tj) {
        __syncthreads();  // the last tile's masks have been read
        if (threadIdx.x < kWave) mask[threadIdx.x] = rank_mask_step(a.eidx, cur, end, tj * kIntTile);
    }
    // after the tile's product: the masks of the lane's eight rows
    __device__ __forceinline__ void rows(unsigned long long (&em)[2][4]) const {
        const int lane = threadIdx.x & 63, wr = threadIdx.x >> 7;
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int r = 0; r < 4; ++r) em[ra][r] = mask[wr * 32 + ra * 16 + (lane >> 4) + 4 * r];
    }
};

template <int MODE, bool EXCL = false>
__global__ __launch_bounds__(kBlock) void rank_tile_kernel(RankArgs a) {
    static_assert(!EXCL || MODE == RANK_SELECT, "only the selection takes an exclusion list");
    extern __shared__ double rank_lds[];
    double* sA = rank_lds;
    double* sB = sA + kIntTile * kIntLd;
    const SelLds s(sB + kIntTile * kIntLd, a.sel.cap);
    [[maybe_unused]] RankExcl ex{reinterpret_cast<unsigned long long*>(s.end())};

    const int strip = blockIdx.x, ti = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int Tc = (a.C + kIntTile - 1) / kIntTile;
    const int t0 = strip * a.strip_tiles;
    const int t1 = (t0 + a.strip_tiles < Tc) ? t0 + a.strip_tiles : Tc;
    const int c0 = t0 * kIntTile;  // first candidate of the strip
    const auto ident = [](double v) { return v; };

    if constexpr (MODE == RANK_SELECT) sel_init(s, -INFINITY);
    // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15
    double rcv[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            rcv[ra][r] = a.rc[(size_t)ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r];
    if constexpr (EXCL) ex.open(a, ti, c0);

    const double* Ug = a.U + (size_t)ti * kIntTile * a.Rp;
    for (int tj = t0; tj < t1; ++tj) {
        if constexpr (EXCL) ex.tile(a, tj);
        int_v4d acc[2][2];
        int_tile_product(Ug, a.V + (size_t)tj * kIntTile * a.Rp, a.Rp, sA, sB, acc);
        [[maybe_unused]] unsigned long long em[2][4];
        if constexpr (EXCL) ex.rows(em);
        // accumulator element (ra, cb, r): its score, and whether the pair exists and is kept
        const auto score = [&](int ra, int cb, int r, double& v) {
            const int bit = wc * 32 + cb * 16 + l15;
            // (cc is padded to whole tiles)
            v = acc[ra][cb][r] + (rcv[ra][r] + a.cc[tj * kIntTile + bit]);
            bool in = ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r < a.nrow &&
                      tj * kIntTile + bit < a.C;
            if constexpr (EXCL) in = in && !((em[ra][r] >> bit) & 1ull);
            return in;
        };
        if constexpr (MODE == RANK_DENSE) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const size_t row = ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
                        double v;
                        if (score(ra, cb, r, v))
                            a.dense[row * a.C + tj * kIntTile + wc * 32 + cb * 16 + l15] = v;
                    }
        } else {
            sel_tile(s, a.sel.K, tj * kIntTile - c0, score, ident);
        }
    }
    if constexpr (MODE == RANK_SELECT)
        sel_write(s, a.sel, strip, ti * kIntTile, a.nrow, a.rows_pad, c0, -INFINITY, ident);
}

// one wave per context row of the slab
static __global__ __launch_bounds__(kBlock) void rank_merge_kernel(RankArgs a) {
    sel_merge(a.sel, a.n_strips, a.nrow, a.rows_pad, [](double v) { return v; },
              [](int32_t c) { return c; }, nullptr);
}

}  // namespace spfm
