// spfm_partners.hip.h -- per-feature views of W = P_o^T diag(lams) P_o: for every feature its
// degree, total and largest weight (spfm_interaction_degrees) and its K strongest partners
// (spfm_interaction_partners, include/spfm.h).  Part of the gfx950 device code of the sparse-FM
// proximal CD core; see DESIGN.md section 14b.
//
// Both walk the full square of W, rows = query features, columns = candidate partners, on the
// compacted images A / B of spfm_interactions.hip.h.  Staging, quadrants and the MFMA chain are
// those of int_tile_kernel (int_stage_chunk / int_mfma_chunk, chunks of 32 components, s = 0, 4,
// 8, ... in order), with the query rows as the A operand and the candidates as the B operand: a
// value of W is the same bits here, in spfm_interaction_topk / _list and under every partition.
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
// 2. part_tile_kernel<PART_SELECT>: rank_tile_kernel<RANK_SELECT>'s scheme (spfm_rank.hip.h) with
//    the signed W in the buffer and the key derived from it (|W|, W or -W: an entry is admissible
//    when its key is > 0, so `thr` starts at 0).  A candidate survives when its key is > thr
//    (candidates come in ascending order: a tie with the K-th loses); rows that cannot take a
//    tile's survivors are compacted first (part_compact: rank_compact on keys).  At the end of the
//    strip every row's sorted list is written out.
//    part_merge_kernel: one wave per query; an entry's final rank is its position in its own list
//    plus, by binary search, the entries of every other list that beat it (key descending, id
//    ascending: a total order, so no result bit depends on the partition).
#pragma once
#include "spfm_interactions.hip.h"
#include "spfm_rank.hip.h"

namespace spfm {

constexpr int kPartMaxK = 128;                  // SPFM_INTERACTION_MAX_K
constexpr int kPartCap = kPartMaxK + kIntTile;  // buffer entries per row: K + one tile's worth
constexpr int kPartMaxStrip = 65536;            // candidates per strip: 16-bit local ids
enum { PART_DEGREE = 0, PART_SELECT = 1 };
enum { PART_ABS = 0, PART_POS = 1, PART_NEG = 2 };
static_assert(kPartCap <= 3 * kWave, "part_compact keeps three entries per lane");

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
    int K, cap, by;
    double tol;
    PartRec* rec;           // PART_DEGREE (rows_pad, t_hi - t_lo)
    double* lval;           // PART_SELECT (n_strips, rows_pad, K): signed W
    int32_t* lidx;          //             compact ranks, INT32_MAX = padding
    double* oval;           // merge (nrow, K)
    int32_t* oidx;
    int32_t* ocnt;          // (nrow)
};

struct PartOut {  // of part_reduce_kernel, per compact rank
    long long* cnt;
    double* sum;
    double* mx;
    int32_t* arg;  // feature id, -1 = none
};

// dynamic LDS of part_tile_kernel<MODE>
static inline size_t part_lds_bytes(int mode, int cap) {
    size_t b = sizeof(double) * 2 * kIntTile * kIntLd;
    if (mode == PART_SELECT)
        b += (size_t)kIntTile * cap * (sizeof(double) + sizeof(uint16_t)) +
             kIntTile * (sizeof(double) + 2 * sizeof(int));
    else
        b += sizeof(PartRec) * 2 * kIntTile;
    return b;
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

// One wave: the n entries of a row's buffer -> its min(n, K) best by key, sorted, at the front
// (rank_compact of spfm_rank.hip.h with the key derived from the stored value)
__device__ __forceinline__ void part_compact(double* bv, uint16_t* bc, int* cnt, double* thr, int K,
                                             int by) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(*cnt);  // wave-uniform
    double w[3], v[3];
    unsigned c[3];
    int rk[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = lane + q * kWave;
        w[q] = i < n ? bv[i] : 0.0;
        v[q] = part_key(w[q], by);
        c[q] = i < n ? bc[i] : 0u;
        rk[q] = 0;
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {  // entry p * 64 + l sits in lane l, slot p
        const int m = n - p * kWave < kWave ? n - p * kWave : kWave;
        for (int l = 0; l < m; ++l) {
            const double vj = readlane_d(v[p], l);
            const unsigned cj = (unsigned)__builtin_amdgcn_readlane((int)c[p], l);
#pragma unroll
            for (int q = 0; q < 3; ++q) rk[q] += rank_beats(vj, cj, v[q], c[q]) ? 1 : 0;
        }
    }
    __builtin_amdgcn_wave_barrier();  // every entry is in registers before the moves
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = lane + q * kWave;
        if (i < n && rk[q] < K) {
            bv[rk[q]] = w[q];
            bc[rk[q]] = (uint16_t)c[q];
            if (rk[q] == K - 1) *thr = v[q];
        }
    }
    if (lane == 0) *cnt = n < K ? n : K;
    __builtin_amdgcn_wave_barrier();
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void part_tile_kernel(PartArgs a) {
    extern __shared__ double part_lds[];
    double* sA = part_lds;
    double* sB = sA + kIntTile * kIntLd;
    // PART_SELECT
    double* bval = sB + kIntTile * kIntLd;                  // [64][cap]
    double* thr = bval + (size_t)kIntTile * a.cap;          // [64]
    uint16_t* bidx = reinterpret_cast<uint16_t*>(thr + kIntTile);  // [64][cap]
    int* cnt = reinterpret_cast<int*>(bidx + (size_t)kIntTile * a.cap);  // [64]
    int* add = cnt + kIntTile;                              // [64] survivors of the tile
    // PART_DEGREE
    PartRec* sRec = reinterpret_cast<PartRec*>(sB + kIntTile * kIntLd);  // [2][64]

    const int strip = blockIdx.x, ti = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int t0 = a.t_lo + strip * a.strip_tiles;
    const int t1 = (t0 + a.strip_tiles < a.t_hi) ? t0 + a.strip_tiles : a.t_hi;
    const int c0 = t0 * kIntTile;  // first candidate of the strip
    const int Tc = a.t_hi - a.t_lo;

    if constexpr (MODE == PART_SELECT) {
        if (threadIdx.x < kIntTile) {
            thr[threadIdx.x] = 0.0;  // a key must be > 0
            cnt[threadIdx.x] = 0;
            add[threadIdx.x] = 0;
        }
    }
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
        int_acc_zero(acc);
        const double* Bg = a.B + (size_t)tj * kIntTile * a.kp;
        for (int kc0 = 0; kc0 < a.kp; kc0 += kIntKC) {
            const int kend = (a.kp - kc0 < kIntKC) ? a.kp - kc0 : kIntKC;  // multiple of 4
            int_stage_chunk(Qg, Bg, a.kp, kc0, kend, sA, sB);
            int_mfma_chunk<false>(sA, sB, kend, nullptr, acc);
        }
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
            // pass 0: count the survivors; pass 1: append
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const int col = tj * kIntTile + wc * 32 + cb * 16 + l15;
                    const bool colin = col >= a.r_lo && col < a.r_hi;
#pragma unroll
                    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int rl = wr * 32 + ra * 16 + l4 + 4 * r;
                            const double w = acc[ra][cb][r];
                            const bool in = colin && col != qr[ra][r];
                            if (in && part_key(w, a.by) > thr[rl]) {
                                if (pass == 0) {
                                    atomicAdd(&add[rl], 1);
                                } else {
                                    const int pos = atomicAdd(&cnt[rl], 1);  // < cap
                                    bval[(size_t)rl * a.cap + pos] = w;
                                    bidx[(size_t)rl * a.cap + pos] = (uint16_t)(col - c0);
                                }
                            }
                        }
                }
                if (pass == 0) {
                    // a row that cannot take its survivors is compacted first: thr rises, and
                    // K + 64 <= cap entries always fit afterwards
                    __syncthreads();
                    for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
                        if (cnt[rl] + add[rl] > a.cap)
                            part_compact(bval + (size_t)rl * a.cap, bidx + (size_t)rl * a.cap,
                                         cnt + rl, thr + rl, a.K, a.by);
                        __builtin_amdgcn_wave_barrier();
                        if (lane == 0) add[rl] = 0;
                    }
                    __syncthreads();
                }
            }
            // (the next tile reads thr / cnt / add behind the barriers of its staging step)
        }
    }
    if constexpr (MODE == PART_SELECT) {
        __syncthreads();
        for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
            const int row = ti * kIntTile + rl;
            if (row >= a.nrow) continue;  // wave-uniform
            part_compact(bval + (size_t)rl * a.cap, bidx + (size_t)rl * a.cap, cnt + rl, thr + rl,
                         a.K, a.by);
            const int n = cnt[rl];
            const size_t o = ((size_t)strip * a.rows_pad + row) * a.K;
            for (int q = lane; q < a.K; q += kWave) {
                a.lval[o + q] = q < n ? bval[(size_t)rl * a.cap + q] : 0.0;
                a.lidx[o + q] = q < n ? c0 + (int)bidx[(size_t)rl * a.cap + q] : INT32_MAX;
            }
        }
    }
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
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= a.nrow) return;  // wave-uniform
    const int K = a.K, N = a.n_strips * K;
    const size_t sstride = (size_t)a.rows_pad * K;
    const double* lv = a.lval + (size_t)row * K;
    const int32_t* li = a.lidx + (size_t)row * K;
    int found = 0;
    for (int e = lane; e < N; e += kWave) {
        const int i = e / K, q = e - i * K;
        const double w = lv[i * sstride + q];
        const int32_t c = li[i * sstride + q];
        if (c == INT32_MAX) continue;  // padding of a short list
        ++found;
        const double v = part_key(w, a.by);
        int rank = q;
        for (int j = 0; j < a.n_strips; ++j) {
            if (j == i) continue;
            const double* jv = lv + j * sstride;
            const int32_t* jc = li + j * sstride;
            int lo = 0, hi = K;  // first entry of list j that does not beat (v, c)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rank_beats(part_key(jv[mid], a.by), (unsigned)jc[mid], v, (unsigned)c))
                    lo = mid + 1;
                else
                    hi = mid;
            }
            rank += lo;
        }
        if (rank < K) {
            a.oval[(size_t)row * K + rank] = w;
            a.oidx[(size_t)row * K + rank] = a.ids[c];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) found += __shfl_xor(found, m, kWave);
    if (lane == 0) a.ocnt[row] = found < K ? found : K;
}

}  // namespace spfm
