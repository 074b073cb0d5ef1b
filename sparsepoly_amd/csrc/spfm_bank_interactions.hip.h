// spfm_bank_interactions.hip.h -- consensus interactions over a model bank: per feature pair
// j < j' the number of members f with |W_f[j, j']| > tol, the number with W_f > tol and the sum of
// the counted W_f, W_f = sum_s lams_s p_sj p_sj' over the member's own components
// (spfm_bank_interaction_*, include/spfm.h).  Part of the gfx950 device code of the sparse-FM
// proximal CD core; see DESIGN.md section 24.
//
// The operand is the resident bank image of one block, feature-major with the members stacked
// along the component axis: element (j, s) at pt[j * S + s], member f the columns
// [koff[f], koff[f + 1]).  Nothing is packed and nothing of size d_u x S or d^2 is stored.
//
// 1. Union compaction.  int_flag_kernel over all S columns marks the features that any member
//    stores a non-zero for; scan and int_compact_kernel give ids[] (spfm_interactions.hip.h).
//    bi_mask_kernel gives every 64-feature tile row the 64-bit set of members with a non-zero in it.
// 2. bi_tile_kernel<MODE>: workgroup t of a launch owns the 64 x 64 tile (ti <= tj) number
//    tile0 + t of the union, in int_tile_kernel's order, wave quadrants and accumulator map.  It
//    walks the members of mask[ti] & mask[tj] in ascending order; a skipped member has an all-zero
//    operand tile, so every value of it is an exact zero and is never counted.  Per member the
//    chunks of 32 components are staged straight from the image through ids[] -- A = the rows of
//    ti, B = lams * the rows of tj -- and go through int_mfma_chunk: W_f[j, j'] is the very chain
//    of v_mfma_f64_16x16x4_f64 steps over s = 0, 4, 8, ... that int_tile_product runs for the
//    member alone (its components padded with zeros to a multiple of 4).
//    The staging is double-buffered over the flattened (member, chunk) sequence: the global loads
//    of step n + 1 are issued into registers ahead of the MFMAs of step n and written to the other
//    LDS buffer behind them; one barrier per step.
//    After a member's last chunk each of the lane's 16 values is thresholded into per-slot state
//    that stays in registers for the whole walk: count | n_pos << 8 in one 32-bit register, one
//    f64 sum (added in member order; one workgroup owns a pair, so no bit depends on the launch
//    partition).  Epilogues:
//      BI_HIST  LDS counters of count = 1..F per tile and of the kept pairs per member (a wave
//               popcount per member inside the walk), flushed with 64-bit integer atomics: exact,
//               order-free
//      BI_EMIT  every pair with count >= min_count appended (wave-aggregated ticket) as key =
//               row id << 32 | column id and {sum, count | n_pos << 8}; the ticket counts ALL such
//               pairs, entries beyond `cap` are dropped
// 3. bi_counts_kernel: the same three numbers at L given pairs, one thread per pair walking the
//    members and their components in order (int_values_kernel's arithmetic per member).
#pragma once
#include "spfm_interactions.hip.h"

namespace spfm {

constexpr int kBiMaxModels = 64;  // = SPFM_BANK_MAX_MODELS: a member per bit of a tile row's mask
enum { BI_HIST = 0, BI_EMIT = 1 };
constexpr int kBiRows = kIntTile * kIntKC / kBlock;  // rows of a chunk per thread and operand

struct BiVal {  // payload of an emitted pair
    double sum;
    uint32_t cn;  // count | n_pos << 8
    uint32_t pad;
};

struct BiArgs {
    const double* pt;     // (d, S): the block's image
    const double* lams;   // (S)
    const int32_t* koff;  // (F + 1)
    const int32_t* ids;   // compact index -> feature id (d_u)
    const unsigned long long* mask;  // (T): members with a non-zero in the tile row
    int S, F, du, T;
    long long tile0;  // first tile of this launch
    double tol;
    int min_count;                 // BI_EMIT
    unsigned long long* hist;      // BI_HIST [F + 1] by count, then [F] kept pairs per member
    unsigned long long cap;        // BI_EMIT
    unsigned long long* counter;
    unsigned long long* keys;
    BiVal* vals;
};

// mask[ti] bit f: member f stores a non-zero for one of the features ids[64 ti .. 64 ti + 63]
static __global__ __launch_bounds__(kBlock) void bi_mask_kernel(
    const double* __restrict__ pt, int S, int F, const int32_t* __restrict__ koff,
    const int32_t* __restrict__ ids, int du, unsigned long long* __restrict__ mask) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * kIntTile;
    unsigned long long m = 0ull;
    for (int f = 0; f < F; ++f) {
        const int k0 = koff[f], k1 = koff[f + 1];
        int any = 0;
        for (int r = wave; r < kIntTile && row0 + r < du; r += kBlock / kWave) {
            const double* row = pt + (size_t)ids[row0 + r] * S;
            for (int s = k0 + lane; s < k1; s += kWave) any |= (row[s] != 0.0) ? 1 : 0;
        }
        if (__syncthreads_or(any)) m |= 1ull << f;
    }
    if (threadIdx.x == 0) mask[blockIdx.x] = m;
}

// components [kc0, kc0 + 32) of member columns [k0, k0 + kf) of the 64 + 64 rows in sId -> registers
// (zeros past the member's components and for the rows past d_u); B carries diag(lams)
__device__ __forceinline__ void bi_load_chunk(const BiArgs& a, const int32_t* sId, int k0, int kf,
                                              int kc0, double (&ra)[kBiRows],
                                              double (&rb)[kBiRows]) {
    const int c = threadIdx.x % kIntKC, r0 = threadIdx.x / kIntKC;
    const bool in = kc0 + c < kf;
    const size_t col = (size_t)k0 + kc0 + c;
    const double l = in ? a.lams[col] : 0.0;
#pragma unroll
    for (int i = 0; i < kBiRows; ++i) {
        const int r = r0 + i * (kBlock / kIntKC);
        const int ja = sId[r], jb = sId[kIntTile + r];
        ra[i] = (in && ja >= 0) ? a.pt[(size_t)ja * a.S + col] : 0.0;
        const double pb = (in && jb >= 0) ? a.pt[(size_t)jb * a.S + col] : 0.0;
        rb[i] = l * pb;
    }
}

__device__ __forceinline__ void bi_store_chunk(const double (&ra)[kBiRows],
                                               const double (&rb)[kBiRows], double* sA,
                                               double* sB) {
    const int c = threadIdx.x % kIntKC, r0 = threadIdx.x / kIntKC;
#pragma unroll
    for (int i = 0; i < kBiRows; ++i) {
        const int r = r0 + i * (kBlock / kIntKC);
        sA[r * kIntLd + c] = ra[i];
        sB[r * kIntLd + c] = rb[i];
    }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void bi_tile_kernel(BiArgs a) {
    __shared__ double sA[2][kIntTile * kIntLd];
    __shared__ double sB[2][kIntTile * kIntLd];
    __shared__ int32_t sId[2 * kIntTile];  // feature ids of the rows of ti, then of tj; -1 past d_u
    __shared__ unsigned sHist[MODE == BI_HIST ? kBiMaxModels + 1 : 1];
    __shared__ unsigned sMem[MODE == BI_HIST ? kBiMaxModels : 1];

    const long long t = a.tile0 + blockIdx.x;
    long long ti, tj;
    int_tile_coords(t, a.T, ti, tj);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;

    if (tid < 2 * kIntTile) {
        const long long jj = (tid < kIntTile ? ti : tj) * kIntTile + (tid & (kIntTile - 1));
        sId[tid] = jj < a.du ? a.ids[jj] : -1;
    }
    if constexpr (MODE == BI_HIST) {
        if (tid <= kBiMaxModels) sHist[tid] = 0u;
        if (tid < kBiMaxModels) sMem[tid] = 0u;
    }
    __syncthreads();

    // the members to walk, in scalar registers
    const unsigned long long m = a.mask[ti] & a.mask[tj];
    unsigned long long rem =
        ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(m >> 32)) << 32) |
        (unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)m);

    // per-slot state: register r of accumulator (ra, cb) is slot (ra * 2 + cb) * 4 + r
    unsigned cn[16];
    double sm[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        cn[q] = 0u;
        sm[q] = 0.0;
    }

    if (rem != 0ull) {
        int f = __ffsll((long long)rem) - 1;
        rem &= rem - 1ull;
        int k0 = a.koff[f], kf = a.koff[f + 1] - k0, kc0 = 0, buf = 0;
        double ra[kBiRows], rb[kBiRows];
        bi_load_chunk(a, sId, k0, kf, kc0, ra, rb);
        bi_store_chunk(ra, rb, sA[0], sB[0]);
        __syncthreads();
        int_v4d acc[2][2];
        for (;;) {
            // the step after this one: the member's next chunk, or the next member's first
            int nf = f, nk0 = k0, nkf = kf, nkc0 = kc0 + kIntKC;
            bool more = true;
            if (nkc0 >= kf) {
                if (rem != 0ull) {
                    nf = __ffsll((long long)rem) - 1;
                    rem &= rem - 1ull;
                    nk0 = a.koff[nf];
                    nkf = a.koff[nf + 1] - nk0;
                    nkc0 = 0;
                } else {
                    more = false;
                }
            }
            if (more) bi_load_chunk(a, sId, nk0, nkf, nkc0, ra, rb);  // in flight over the MFMAs
            if (kc0 == 0) int_acc_zero(acc);
            const int kp = (kf + 3) & ~3;
            const int kend = (kp - kc0 < kIntKC) ? kp - kc0 : kIntKC;  // multiple of 4
            int_mfma_chunk<false>(sA[buf], sB[buf], kend, nullptr, acc);
            if (kc0 + kIntKC >= kf) {  // the member's last chunk: its values are complete
                // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15
                unsigned kept = 0u;
#pragma unroll
                for (int qa = 0; qa < 2; ++qa)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int q = (qa * 2 + cb) * 4 + r;
                            const long long gi = ti * kIntTile + wr * 32 + qa * 16 + l4 + 4 * r;
                            const long long gj = tj * kIntTile + wc * 32 + cb * 16 + l15;
                            const double w = acc[qa][cb][r];
                            const bool take = gi < gj && fabs(w) > a.tol;  // diagonal tile: j < j'
                            if (take) {
                                cn[q] += (w > 0.0) ? 0x101u : 0x001u;
                                sm[q] += w;
                            }
                            if constexpr (MODE == BI_HIST)
                                kept += (unsigned)__popcll(__ballot(take));
                        }
                if constexpr (MODE == BI_HIST) {
                    if (lane == 0 && kept) atomicAdd(&sMem[f], kept);
                }
            }
            if (more) bi_store_chunk(ra, rb, sA[buf ^ 1], sB[buf ^ 1]);
            __syncthreads();
            if (!more) break;
            buf ^= 1;
            f = nf;
            k0 = nk0;
            kf = nkf;
            kc0 = nkc0;
        }
    }

    if constexpr (MODE == BI_HIST) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const unsigned c = cn[q] & 0xffu;
            if (c) atomicAdd(&sHist[c], 1u);
        }
        __syncthreads();
        if (tid >= 1 && tid <= a.F && sHist[tid])
            atomicAdd(&a.hist[tid], (unsigned long long)sHist[tid]);
        if (tid < a.F && sMem[tid])
            atomicAdd(&a.hist[a.F + 1 + tid], (unsigned long long)sMem[tid]);
    } else {
#pragma unroll
        for (int qa = 0; qa < 2; ++qa)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = (qa * 2 + cb) * 4 + r;
                    const bool take = (int)(cn[q] & 0xffu) >= a.min_count;  // (min_count >= 1)
                    const unsigned long long bal = __ballot(take);
                    if (bal != 0ull) {  // wave-uniform
                        const int leader = __ffsll((long long)bal) - 1;
                        unsigned long long slot = 0ull;
                        if (lane == leader)
                            slot = atomicAdd(a.counter, (unsigned long long)__popcll(bal));
                        slot = __shfl(slot, leader, kWave);
                        if (take) {
                            slot += (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
                            if (slot < a.cap) {
                                const int li = wr * 32 + qa * 16 + l4 + 4 * r;
                                const int lj = wc * 32 + cb * 16 + l15;
                                a.keys[slot] =
                                    ((unsigned long long)(unsigned)sId[li] << 32) |
                                    (unsigned long long)(unsigned)sId[kIntTile + lj];
                                a.vals[slot] = BiVal{sm[q], cn[q], 0u};
                            }
                        }
                    }
                }
    }
}

// the three numbers at L pairs: one thread per pair, members in order, components in order;
// j == j' gives zeros (no diagonal)
static __global__ __launch_bounds__(kBlock) void bi_counts_kernel(
    const double* __restrict__ pt, int S, int F, const int32_t* __restrict__ koff,
    const double* __restrict__ lams, double tol, long long L, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ cols, int32_t* __restrict__ count, int32_t* __restrict__ n_pos,
    double* __restrict__ sum) {
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (q >= L) return;
    const double* pj = pt + (size_t)rows[q] * S;
    const double* pj2 = pt + (size_t)cols[q] * S;
    int c = 0, np = 0;
    double sm = 0.0;
    if (rows[q] != cols[q])
        for (int f = 0; f < F; ++f) {
            double w = 0.0;
            for (int s = koff[f]; s < koff[f + 1]; ++s) w += (lams[s] * pj[s]) * pj2[s];
            if (fabs(w) > tol) {
                ++c;
                np += (w > 0.0) ? 1 : 0;
                sm += w;
            }
        }
    count[q] = c;
    n_pos[q] = np;
    sum[q] = sm;
}

}  // namespace spfm
