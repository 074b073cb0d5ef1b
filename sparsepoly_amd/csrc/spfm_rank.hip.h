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
//    candidate tiles of its strip, one after the other.  Staging, quadrants and the MFMA chain
//    are those of int_tile_kernel (spfm_interactions.hip.h: int_stage_chunk / int_mfma_chunk,
//    chunks of 32 columns, s = 0, 4, 8, ... in order); a score is acc + (rowconst + colconst),
//    the same bits in every mode and under every slab / strip partition.
//      RANK_DENSE   stores the tile
//      RANK_SELECT  keeps per context row, in LDS, the K-th best value seen so far (`thr`) and a
//                   buffer of kRankCap = 192 (value, strip-local candidate) entries: 10 bytes each,
//                   64 rows, 120 KiB beside the 36 KiB of staging.  A score is a survivor when it
//                   is > thr (candidates come in ascending order, so a tie with the K-th loses
//                   under the tie rule).  Per tile: the survivors of every row are counted
//                   (integer LDS counters); a row whose buffer could not take them is compacted
//                   first -- that raises its thr, and K + 64 <= 192 always fits afterwards --; then
//                   the survivors of the current thr are appended.  Compaction, by one wave: every
//                   entry is ranked by counting the entries that beat it (value descending,
//                   candidate ascending: a total order, so the outcome does not depend on the order
//                   of the appends; the entries travel through lane broadcasts, not LDS), the K best
//                   move to their rank, thr becomes the K-th.  A compaction thus absorbs up to
//                   192 - K survivors.  At the end of the strip every row is compacted and its
//                   sorted list written out.
//      RANK_MERGE   one wave per context row: an entry's final rank is its position in its own
//                   strip's list plus, by binary search, the entries of every other list that beat
//                   it; ranks below K are written.
//    No float atomics; the LDS counters are integers.  Non-finite scores never enter a list.
//    EXCL (spfm_rank_topk_excl): per context row an ascending list of
//    candidates that are left out.  Before a tile is staged, wave 0 (lane = row of the tile)
//    turns each row's list into one 64-bit mask of the tile's columns (rank_mask_step: a cursor per
//    row, kept across the tiles of the strip, found by binary search where the strip starts); the
//    masks sit in LDS (512 B) and a score survives only if its bit is clear.  EXCL = false is the
//    code without any of this.
#pragma once
#include "spfm_interactions.hip.h"

namespace spfm {

constexpr int kRankMaxK = 128;                    // SPFM_RANK_MAX_K
constexpr int kRankCap = kRankMaxK + kIntTile;    // buffer entries per row: K + one tile's worth
constexpr int kRankMaxStrip = 65536;              // candidates per strip: 16-bit local ids
enum { RANK_DENSE = 0, RANK_SELECT = 1, RANK_MERGE = 2 };
enum { RANK_CTX = 0, RANK_CAND = 1 };
static_assert(kRankCap <= 3 * kWave, "rank_compact keeps three entries per lane");

struct RankArgs {
    const double* U;    // (rows padded, Rp) of the slab
    const double* V;    // (candidates padded, Rp)
    const double* rc;   // rowconst of the slab (padded)
    const double* cc;   // colconst (padded)
    int Rp, nrow, C;    // padded columns; context rows of the slab; candidates
    int strip_tiles, n_strips, rows_pad;
    int K, cap;         // list length min(K, C); buffer entries per row
    double* dense;      // RANK_DENSE (nrow, C)
    double* lval;       // RANK_SELECT / RANK_MERGE (n_strips, rows_pad, K)
    int32_t* lidx;
    double* oval;       // RANK_MERGE (nrow, K)
    int32_t* oidx;
    const int64_t* eptr;  // EXCL: excluded candidates of every context row of the call (CSR
    const int32_t* eidx;  //       pattern, ascending per row), row `row0 + r` for slab row r
    int64_t row0;
};

// dynamic LDS of rank_tile_kernel<MODE>
static inline size_t rank_lds_bytes(int mode, int cap, bool excl = false) {
    size_t b = sizeof(double) * 2 * kIntTile * kIntLd;
    if (mode == RANK_SELECT)
        b += (size_t)kIntTile * cap * (sizeof(double) + sizeof(uint16_t)) +
             kIntTile * (sizeof(double) + 2 * sizeof(int)) +
             (excl ? kIntTile * sizeof(unsigned long long) : 0);
    return mode == RANK_MERGE ? 0 : b;
}

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
        if constexpr (M == 0) {
            double a = 1.0;
            for (int64_t ii = b; ii < e; ++ii)
                a *= 1 + (double)rval[ii] * base[s * ss + (int64_t)ridx[ii] * sj];
            out[s] = (side == RANK_CTX) ? lam * a : a;
        } else {
            double a[M + 1];
            a[0] = 1.0;
#pragma unroll
            for (int t = 1; t <= M; ++t) a[t] = 0.0;
            for (int64_t ii = b; ii < e; ++ii) {
                const double px = base[s * ss + (int64_t)ridx[ii] * sj] * (double)rval[ii];
#pragma unroll
                for (int t = M; t >= 1; --t) a[t] += a[t - 1] * px;
            }
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

// (value descending, candidate ascending)
__device__ __forceinline__ bool rank_beats(double va, unsigned ca, double vb, unsigned cb) {
    return va > vb || (va == vb && ca < cb);
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

// One wave: the n entries of a row's buffer -> its min(n, K) best, sorted, at the front
__device__ __forceinline__ void rank_compact(double* bv, uint16_t* bc, int* cnt, double* thr,
                                             int K) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(*cnt);  // wave-uniform
    double v[3];
    unsigned c[3];
    int rk[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = lane + q * kWave;
        v[q] = i < n ? bv[i] : 0.0;
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
            bv[rk[q]] = v[q];
            bc[rk[q]] = (uint16_t)c[q];
            if (rk[q] == K - 1) *thr = v[q];
        }
    }
    if (lane == 0) *cnt = n < K ? n : K;
    __builtin_amdgcn_wave_barrier();
}

template <int MODE>
__device__ __forceinline__ void rank_merge_body(const RankArgs& a) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= a.nrow) return;
    const int K = a.K, N = a.n_strips * K;
    const size_t sstride = (size_t)a.rows_pad * K;
    const double* lv = a.lval + (size_t)row * K;
    const int32_t* li = a.lidx + (size_t)row * K;
    for (int e = lane; e < N; e += kWave) {
        const int i = e / K, q = e - i * K;
        const double v = lv[i * sstride + q];
        const int32_t c = li[i * sstride + q];
        if (c == INT32_MAX) continue;  // padding of a short list
        int rank = q;
        for (int j = 0; j < a.n_strips; ++j) {
            if (j == i) continue;
            const double* jv = lv + j * sstride;
            const int32_t* jc = li + j * sstride;
            int lo = 0, hi = K;  // first entry of list j that does not beat (v, c)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rank_beats(jv[mid], (unsigned)jc[mid], v, (unsigned)c))
                    lo = mid + 1;
                else
                    hi = mid;
            }
            rank += lo;
        }
        if (rank < K) {
            a.oval[(size_t)row * K + rank] = v;
            a.oidx[(size_t)row * K + rank] = c;
        }
    }
}

template <int MODE, bool EXCL = false>
__global__ __launch_bounds__(kBlock) void rank_tile_kernel(RankArgs a) {
    static_assert(!EXCL || MODE == RANK_SELECT, "only the selection takes an exclusion list");
    if constexpr (MODE == RANK_MERGE) {
        rank_merge_body<MODE>(a);
        return;
    } else {
        extern __shared__ double rank_lds[];
        double* sA = rank_lds;
        double* sB = sA + kIntTile * kIntLd;
        double* bval = sB + kIntTile * kIntLd;                  // [64][cap]
        double* thr = bval + (size_t)kIntTile * a.cap;          // [64]
        uint16_t* bidx = reinterpret_cast<uint16_t*>(thr + kIntTile);  // [64][cap]
        int* cnt = reinterpret_cast<int*>(bidx + (size_t)kIntTile * a.cap);  // [64]
        int* add = cnt + kIntTile;                              // [64] survivors of the tile
        [[maybe_unused]] unsigned long long* emask =
            reinterpret_cast<unsigned long long*>(add + kIntTile);  // [64] EXCL

        const int strip = blockIdx.x, ti = blockIdx.y;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int wr = wave >> 1, wc = wave & 1;
        const int l15 = lane & 15, l4 = lane >> 4;
        const int Tc = (a.C + kIntTile - 1) / kIntTile;
        const int t0 = strip * a.strip_tiles;
        const int t1 = (t0 + a.strip_tiles < Tc) ? t0 + a.strip_tiles : Tc;
        const int c0 = t0 * kIntTile;  // first candidate of the strip

        if constexpr (MODE == RANK_SELECT) {
            if (threadIdx.x < kIntTile) {
                thr[threadIdx.x] = -INFINITY;
                cnt[threadIdx.x] = 0;
                add[threadIdx.x] = 0;
            }
        }
        // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15
        double rcv[2][4];
#pragma unroll
        for (int ra = 0; ra < 2; ++ra)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                rcv[ra][r] = a.rc[(size_t)ti * kIntTile + wr * 32 + ra * 16 + l4 + 4 * r];

        // EXCL, wave 0: the row's cursor into eidx, at the strip's first candidate
        [[maybe_unused]] int64_t ecur = 0, eend = 0;
        if constexpr (EXCL) {
            if (wave == 0 && ti * kIntTile + lane < a.nrow) {
                const int64_t row = a.row0 + ti * kIntTile + lane;
                eend = a.eptr[row + 1];
                ecur = rank_lower_bound(a.eidx, a.eptr[row], eend, c0);
            }
        }

        const double* Ug = a.U + (size_t)ti * kIntTile * a.Rp;
        for (int tj = t0; tj < t1; ++tj) {
            if constexpr (EXCL) {
                __syncthreads();  // the last tile's masks have been read
                if (wave == 0) emask[lane] = rank_mask_step(a.eidx, ecur, eend, tj * kIntTile);
                // (published by the barriers of the staging step)
            }
            int_v4d acc[2][2];
            int_acc_zero(acc);
            const double* Vg = a.V + (size_t)tj * kIntTile * a.Rp;
            for (int kc0 = 0; kc0 < a.Rp; kc0 += kIntKC) {
                const int kend = (a.Rp - kc0 < kIntKC) ? a.Rp - kc0 : kIntKC;  // multiple of 4
                int_stage_chunk(Ug, Vg, a.Rp, kc0, kend, sA, sB);
                int_mfma_chunk<false>(sA, sB, kend, nullptr, acc);
            }
            [[maybe_unused]] unsigned long long em[2][4];  // EXCL: the masks of the lane's eight rows
            if constexpr (EXCL) {
#pragma unroll
                for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                    for (int r = 0; r < 4; ++r) em[ra][r] = emask[wr * 32 + ra * 16 + l4 + 4 * r];
            }
            // pass 0: count the survivors (RANK_SELECT); pass 1: store / append
#pragma unroll
            for (int pass = (MODE == RANK_SELECT ? 0 : 1); pass < 2; ++pass) {
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const int col = tj * kIntTile + wc * 32 + cb * 16 + l15;
                    const double ccv = a.cc[col];  // padded to whole tiles
#pragma unroll
                    for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int rl = wr * 32 + ra * 16 + l4 + 4 * r;
                            const int row = ti * kIntTile + rl;
                            const double v = acc[ra][cb][r] + (rcv[ra][r] + ccv);
                            bool in = row < a.nrow && col < a.C;
                            if constexpr (EXCL)
                                in = in && !((em[ra][r] >> (wc * 32 + cb * 16 + l15)) & 1ull);
                            if constexpr (MODE == RANK_DENSE) {
                                if (in) a.dense[(size_t)row * a.C + col] = v;
                            } else {
                                if (in && v > thr[rl]) {
                                    if (pass == 0) {
                                        atomicAdd(&add[rl], 1);
                                    } else {
                                        const int pos = atomicAdd(&cnt[rl], 1);  // < cap
                                        bval[(size_t)rl * a.cap + pos] = v;
                                        bidx[(size_t)rl * a.cap + pos] = (uint16_t)(col - c0);
                                    }
                                }
                            }
                        }
                }
                if constexpr (MODE == RANK_SELECT) {
                    if (pass == 0) {
                        // a row that cannot take its survivors is compacted first: thr rises, and
                        // K + 64 <= cap entries always fit afterwards
                        __syncthreads();
                        for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
                            if (cnt[rl] + add[rl] > a.cap)
                                rank_compact(bval + (size_t)rl * a.cap, bidx + (size_t)rl * a.cap,
                                             cnt + rl, thr + rl, a.K);
                            __builtin_amdgcn_wave_barrier();
                            if (lane == 0) add[rl] = 0;
                        }
                        __syncthreads();
                    }
                }
            }
            // (the next tile reads thr / cnt / add behind the barriers of its staging step)
        }
        if constexpr (MODE == RANK_SELECT) {
            __syncthreads();
            for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
                const int row = ti * kIntTile + rl;
                if (row >= a.nrow) continue;  // wave-uniform
                rank_compact(bval + (size_t)rl * a.cap, bidx + (size_t)rl * a.cap, cnt + rl,
                             thr + rl, a.K);
                const int n = cnt[rl];
                const size_t o = ((size_t)strip * a.rows_pad + row) * a.K;
                for (int q = lane; q < a.K; q += kWave) {
                    a.lval[o + q] = q < n ? bval[(size_t)rl * a.cap + q] : -INFINITY;
                    a.lidx[o + q] = q < n ? c0 + (int)bidx[(size_t)rl * a.cap + q] : INT32_MAX;
                }
            }
        }
    }
}

}  // namespace spfm
