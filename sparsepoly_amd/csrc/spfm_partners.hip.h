// spfm_partners.hip.h -- per-feature views of W = P_o^T diag(lams) P_o: for every feature its
// degree, total and largest weight (spfm_interaction_degrees) and its K strongest partners
// (spfm_interaction_partners, include/spfm.h).  Part of the gfx950 device code of the sparse-FM
// proximal CD core; see DESIGN.md section 14b.
//
// Both walk the full square of W, rows = query features, columns = candidate partners, on the
// compacted images A / B of spfm_interactions.hip.h.  The tile product is int_tile_product, with
// the query rows as the A operand and the candidates as the B operand: a value of W is the same
// bits here, in spfm_interaction_topk / _list and under every partition.
// Workgroup (strip, ti) owns the 64-row query tile ti against the candidate tiles of its strip, in
// ascending order.  The diagonal is masked by comparing compact ranks.
//
// 1. part_tile_kernel<PART_DEGREE>: per (row, candidate tile) one record (count of |W| > tol,
//    sum |W|, max |W|, smallest column attaining it), reduced in a fixed order: the lane's two
//    column blocks in order, the 16 lanes of a quadrant row (xor shuffle tree), the two column
//    quadrants in order.  The record goes to rec[row][tile]; nothing is accumulated across tiles
//    here, so the strip width decides nothing but who computes a record.
//    part_reduce_kernel: one wave per row; lane l combines the tiles l, l + 64, ... in order, then
//    the lanes (xor shuffle tree).  The tree depends on the tile count alone.  No float atomics.
// 2. part_tile_kernel<PART_SELECT>: the streaming top-K selection of spfm_select.hip.h with the
//    signed W in the buffer and the key derived from it (|W|, W or -W: an entry is admissible
//    when its key is > 0, so the floor is 0).
//    part_merge_kernel: sel_merge of the per-strip lists, one wave per query; compact ranks
//    become feature ids and the row's count is written.
#pragma once
#include "spfm_select.hip.h"

namespace spfm {

constexpr int kPartMaxK = kSelMaxK;  // SPFM_INTERACTION_MAX_K
enum { PART_DEGREE = 0, PART_SELECT = 1 };
enum { PART_ABS = 0, PART_POS = 1, PART_NEG = 2 };

struct PartRec {
    double sum, mx;
    int32_t cnt, arg;  // arg: compact rank of the smallest column attaining mx (INT32_MAX: none)
};

struct PartArgs {
    const double* Q;        // query image (rows padded to 64, kp): rows of A, zero rows
    const double* B;        // candidates: the whole packed image
    const int32_t* qrank;   // PART_SELECT: compact rank of every query row, -1 = inactive / padding
    const int32_t* ids;     // compact rank -> feature id
    int kp, nrow, rows_pad; // padded components; query rows of the slab
    int row0;               // PART_DEGREE: compact rank of the slab's first row
    int r_lo, r_hi;         // candidates: compact ranks [r_lo, r_hi)
    int t_lo, t_hi;         // the candidate tiles that hold them
    int strip_tiles, n_strips;
    int by;
    double tol;
    PartRec* rec;           // PART_DEGREE (rows_pad, t_hi - t_lo)
    SelLists sel;           // PART_SELECT, merge: signed W and compact ranks
    int32_t* ocnt;          // merge (nrow)
};

struct PartOut {  // of part_reduce_kernel, per compact rank
    long long* cnt;
    double* sum;
    double* mx;
    int32_t* arg;  // feature id, -1 = none
};

// dynamic LDS of part_tile_kernel<PART_DEGREE> (PART_SELECT: SelPlan::lds)
static inline size_t part_degree_lds_bytes() {
    return int_stage_lds_bytes() + sizeof(PartRec) * 2 * kIntTile;
}

__device__ __forceinline__ double part_key(double w, int by) {
    return by == PART_ABS ? fabs(w) : (by == PART_POS ? w : -w);
}

// (larger maximum; among equal maxima the smaller column)
__device__ __forceinline__ void part_rec_combine(PartRec& a, const PartRec& b) {
    a.cnt += b.cnt;
    a.sum += b.sum;
    const bool take = b.mx > a.mx || (b.mx == a.mx && b.arg < a.arg);
    a.mx = take ? b.mx : a.mx;
    a.arg = take ? b.arg : a.arg;
}

// xor shuffle tree over the lanes whose ids differ in the bits below `width`: every lane of the
// group ends up with the same record (the operations commute exactly)
template <int WIDTH>
__device__ __forceinline__ void part_rec_tree(PartRec& a) {
#pragma unroll
    for (int m = 1; m < WIDTH; m <<= 1) {
        PartRec b;
        b.cnt = __shfl_xor(a.cnt, m, kWave);
        b.arg = __shfl_xor(a.arg, m, kWave);
        b.sum = __shfl_xor(a.sum, m, kWave);
        b.mx = __shfl_xor(a.mx, m, kWave);
        part_rec_combine(a, b);
    }
}

// query image of a slab: row q is the A row of feature J[q] (J NULL: feature j0 + q), zeros for a
// feature that is inactive or out of view and for the padding rows
static __global__ __launch_bounds__(kBlock) void part_gather_kernel(
    const double* __restrict__ A, int kp, const int32_t* __restrict__ flag,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ J, int j0, int nrow, int64_t total,
    double* __restrict__ Q, int32_t* __restrict__ qrank) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const int64_t q = e / kp;
    const int s = (int)(e - q * kp);
    int r = -1;
    if (q < nrow) {
        const int j = J ? J[q] : j0 + (int)q;
        if (flag[j]) r = pos[j];
    }
    Q[e] = r >= 0 ? A[(size_t)r * kp + s] : 0.0;
    if (s == 0) qrank[q] = r;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void part_tile_kernel(PartArgs a) {
    extern __shared__ double part_lds[];
    double* sA = part_lds;
    double* sB = sA + kIntTile * kIntLd;
    const SelLds s(sB + kIntTile * kIntLd, a.sel.cap);                   // PART_SELECT
    PartRec* sRec = reinterpret_cast<PartRec*>(sB + kIntTile * kIntLd);  // PART_DEGREE [2][64]

    const int strip = blockIdx.x, ti = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int t0 = a.t_lo + strip * a.strip_tiles;
    const int t1 = (t0 + a.strip_tiles < a.t_hi) ? t0 + a.strip_tiles : a.t_hi;
    const int c0 = t0 * kIntTile;  // first candidate of the strip
    const int Tc = a.t_hi - a.t_lo;
    const auto key = [by = a.by](double w) { return part_key(w, by); };

    if constexpr (MODE == PART_SELECT) sel_init(s, 0.0);  // a key must be > 0
    // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15.
    // The compact ranks of the lane's eight rows:
    int qr[2][4];
#pragma unroll
    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r;
            qr[ra][r] = (MODE == PART_SELECT) ? a.qrank[row] : a.row0 + row;
        }

    const double* Qg = a.Q + (size_t)ti * kIntTile * a.kp;
    for (int tj = t0; tj < t1; ++tj) {
        int_v4d acc[2][2];
        int_tile_product(Qg, a.B + (size_t)tj * kIntTile * a.kp, a.kp, sA, sB, acc);
        if constexpr (MODE == PART_DEGREE) {
            // (padding rows and columns are zero rows of the images: W = 0 there)
#pragma unroll
            for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    PartRec mine;
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        const int col = tj * kIntTile + wc * 32 + cb * 16 + l15;
                        const double m = (col != qr[ra][r]) ? fabs(acc[ra][cb][r]) : 0.0;
                        PartRec b;
                        b.cnt = (m > a.tol) ? 1 : 0;
                        b.sum = m;
                        b.mx = m;
                        b.arg = (m > 0.0) ? col : INT32_MAX;
                        if (cb == 0)
                            mine = b;
                        else
                            part_rec_combine(mine, b);
                    }
                    part_rec_tree<16>(mine);
                    if (l15 == 0) sRec[wc * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r] = mine;
                }
            __syncthreads();
            if (threadIdx.x < kIntTile) {
                PartRec rec = sRec[threadIdx.x];
                part_rec_combine(rec, sRec[kIntTile + threadIdx.x]);
                a.rec[((size_t)ti * kIntTile + threadIdx.x) * Tc + (tj - a.t_lo)] = rec;
            }
            // (sRec is rewritten behind the barriers of the next tile's staging step)
        } else {
            // admissible: in the candidate range and off the diagonal
            sel_tile(s, a.sel.K, tj * kIntTile - c0,
                     [&](int ra, int cb, int r, double& w) {
                         const int col = tj * kIntTile + wc * 32 + cb * 16 + l15;
                         w = acc[ra][cb][r];
                         return col >= a.r_lo && col < a.r_hi && col != qr[ra][r];
                     },
                     key);
        }
    }
    if constexpr (MODE == PART_SELECT)
        sel_write(s, a.sel, strip, ti * kIntTile, a.nrow, a.rows_pad, c0, 0.0, key);
}

// rows [0, nrow) of a degree slab: the records of the Tc tiles -> the row's answer at compact
// rank row0 + row
static __global__ __launch_bounds__(kBlock) void part_reduce_kernel(
    const PartRec* __restrict__ rec, int nrow, int Tc, int row0, const int32_t* __restrict__ ids,
    PartOut out) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= nrow) return;  // wave-uniform
    PartRec a;
    a.cnt = 0;
    a.sum = a.mx = 0.0;
    a.arg = INT32_MAX;
    // a row has at most 2^31 - 1 partners: the 32-bit counts cannot overflow
    for (int t = lane; t < Tc; t += kWave) part_rec_combine(a, rec[(size_t)row * Tc + t]);
    part_rec_tree<kWave>(a);
    if (lane == 0) {
        out.cnt[row0 + row] = a.cnt;
        out.sum[row0 + row] = a.sum;
        out.mx[row0 + row] = a.mx;
        out.arg[row0 + row] = (a.arg == INT32_MAX) ? -1 : ids[a.arg];
    }
}

// one wave per query row of the slab
static __global__ __launch_bounds__(kBlock) void part_merge_kernel(PartArgs a) {
    sel_merge(a.sel, a.n_strips, a.nrow, a.rows_pad,
              [by = a.by](double w) { return part_key(w, by); },
              [ids = a.ids](int32_t c) { return ids[c]; }, a.ocnt);
}

}  // namespace spfm
