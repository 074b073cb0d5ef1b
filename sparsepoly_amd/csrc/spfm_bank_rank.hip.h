// spfm_bank_rank.hip.h -- the exact ROC-AUC of every member of a bank on sets of rows
// (spfm_bank_group_auc).  Part of the gfx950 device code, behind
// bank_predict_kernel (spfm_bank.hip.h), which it leaves untouched.
//
// Layout.  Resident for one call, member-major: key[f][i] the order-preserving 64-bit image of
// score_if (i the global row), meta[f][i] = group_i << 1 | (y_if > 0), one byte; row[i] = i, the
// payload of every sort; weight[i].  After the last slab member f's keys are sorted (stable radix
// sort) into skey / srow: position p holds the p-th smallest score and its row, equal scores in row
// order.  A tie run is a maximal stretch of equal keys; its last position is its tail.
//
// The statistic.  For one member and one set (a bitmask over the groups), with w_p the weight of
// the row at position p where that row is in the set and 0 where it is not (1 / 0 unweighted):
//   Ninc(p) = the weights of the negatives at positions <= p,
//   Nst(t)  = Ninc at the tail before t's run (0 for the first run): the negatives below the run,
//   Prun(t) = the weights of the positives in t's run,
//   S       = sum over the tails t of  Prun(t) * (Nst(t) + Ninc(t)).
// A positive of run t has Nst(t) negatives below it and Ninc(t) - Nst(t) tied with it, so
//   S = 2 sum_p w_p (sum_{q: s_q < s_p} w_q + 1/2 sum_{q: s_q == s_p} w_q):
// unweighted S is U2 of the header, weighted auc = 0.5 S / (W_pos W_neg).  Every addend and every
// factor is non-negative: there is no subtraction anywhere, so the relative error of S and of the
// two class weights is bounded by the number of additions on the longest path times 2^-53 whatever
// the data; the integer instantiation is exact.
//
// Work split.  The sorted positions go in blocks of kRankBlock; one workgroup of one wavefront per
// (block, member).  The wave stages its block's bytes (meta | tail << 7) and weights in LDS; then
// lane u < U is set u and walks the block's positions one after the other, its state in five
// scalars.  All lanes read the same LDS address (a broadcast); the per-set state is never an array.
// The tail flag of a position compares its key with the next position's, read from memory (so the
// last position of a block looks into the next block).  Three launches per batch of members:
//   bank_rank_block_kernel  per block, from zero: Nloc, Ploc (the block's negatives / positives),
//                           whether it holds a tail, Nloc at its last tail, the positives behind it;
//   bank_rank_carry_kernel  one thread per (member, set), the blocks in order: replaces each
//                           block's record by what enters the block -- Nin (negatives before it),
//                           Nst and Prun of the run that is open at its start -- and gives W_pos,
//                           W_neg; then, called again after the next kernel (phase 1), adds the
//                           blocks' S_b in block order;
//   bank_rank_finish_kernel per block: the walk again with the carry, S_b from zero.
//
// Summation order (a function of the sorted position alone; weighted and unweighted alike).
//   local(p)  = ((0 + w_b0) + w_b1) + ...        negatives of p's block up to p, in position order;
//   Nin(b)    = ((0 + Nloc_0) + Nloc_1) + ...    the blocks before b, in block order;
//   Ninc(p)   = Nin(b) + local(p);   Nst(t) = that value at the tail before t's run;
//   Prun(t)   = ((c + w_r0) + w_r1) + ...        the run's positives in position order, where c is 0
//               for a run that starts in t's block and else Prun carried into the block: the sum,
//               block after block in block order, of the positives ((0 + w) + w) ... of the run's
//               stretch in each earlier block;
//   S_b       = ((0 + T_t0) + T_t1) + ...        T_t = Prun(t) * (Nst(t) + Ninc(t)), the tails of
//               block b in position order;   S = ((0 + S_0) + S_1) + ...  in block order;
//   W_pos     = ((0 + Ploc_0) + Ploc_1) + ...,  W_neg = Nin(last) + Nloc_last.
// A term goes through at most kRankBlock + n / kRankBlock + 3 additions.  Nothing depends on the
// slabs, on F, on the member's position or on the batch; a row of weight 0 adds exact zeros.
#pragma once
#include "spfm_common.hip.h"

#include <type_traits>

namespace spfm {

constexpr int kBankMaxSets = 32;
constexpr int kRankBlock = 256;   // sorted positions per workgroup of the walk
constexpr int kRankThreads = 64;  // one wavefront: lane u is set u
constexpr int kRankTile = 64;     // rows per workgroup of the key kernel
constexpr int kRankRec = 5;       // values per (member, set, block) record
constexpr int kRankMaxModels = 64;  // SPFM_BANK_MAX_MODELS: the members of the key kernel's tile

// the order-preserving unsigned image of a finite double; -0.0 and +0.0 share one key
__device__ __forceinline__ uint64_t rank_key_dev(double s) {
    uint64_t b = (uint64_t)__double_as_longlong(s);
    if (s == 0.0) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

static __global__ __launch_bounds__(kBlock) void bank_rank_iota_kernel(int64_t n,
                                                                       uint32_t* __restrict__ row) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) row[i] = (uint32_t)i;
}

// One slab's scores (rows x F, row-major: read coalesced) into the member-major images, through an
// LDS tile of kRankTile rows so that the writes run along the rows of one member.  y and group are
// the slab's own (row 0 = global row r0).
static __global__ __launch_bounds__(kBlock) void bank_rank_key_kernel(
    int64_t rows, int64_t r0, int64_t n, int F, const double* __restrict__ sc,
    const double* __restrict__ y, int ys_row, int ys_f, const int32_t* __restrict__ group /* or NULL */,
    uint64_t* __restrict__ key /* F x n */, uint8_t* __restrict__ meta /* F x n */) {
    __shared__ uint64_t tile[kRankMaxModels][kRankTile + 1];  // [f][i]
    const int64_t i0 = (int64_t)blockIdx.x * kRankTile;
    const int len = (int)min((int64_t)kRankTile, rows - i0);
    const double* src = sc + (size_t)i0 * F;
    for (int c = threadIdx.x; c < len * F; c += kBlock) {
        const int i = c / F, f = c - i * F;
        tile[f][i] = rank_key_dev(src[c]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < F * kRankTile; c += kBlock) {
        const int f = c / kRankTile, i = c % kRankTile;
        if (i >= len) continue;
        const int64_t r = i0 + i;
        const size_t at = (size_t)f * n + (size_t)(r0 + r);
        const int g = group ? group[r] : 0;  // in [0, 32): checked on the host
        const int pos = y[(size_t)r * ys_row + (size_t)f * ys_f] > 0 ? 1 : 0;
        key[at] = tile[f][i];
        meta[at] = (uint8_t)((g << 1) | pos);
    }
}

// the block's positions into LDS: s_meta[j] = meta of the row | tail << 7, s_w[j] its weight
template <typename A>
__device__ __forceinline__ int rank_stage_dev(int64_t n, int64_t p0, const uint64_t* __restrict__ skey,
                                              const uint32_t* __restrict__ srow,
                                              const uint8_t* __restrict__ meta,
                                              const double* __restrict__ weight, uint8_t* s_meta,
                                              double* s_w) {
    const int len = (int)min((int64_t)kRankBlock, n - p0);
    for (int j = threadIdx.x; j < len; j += kRankThreads) {
        const int64_t p = p0 + j;
        const uint32_t r = srow[p];
        const bool tail = p + 1 == n || skey[p + 1] != skey[p];
        s_meta[j] = (uint8_t)(meta[r] | (tail ? 0x80 : 0));
        if constexpr (std::is_same<A, double>::value) s_w[j] = weight[r];
    }
    __syncthreads();
    return len;
}

// the weight of position j for the set `mask`: 0 outside the set
template <typename A>
__device__ __forceinline__ A rank_weight_dev(uint32_t mask, int m, const double* s_w, int j) {
    const bool in = (mask >> ((m >> 1) & 31)) & 1u;
    if constexpr (std::is_same<A, double>::value)
        return in ? s_w[j] : 0.0;
    else
        return in ? 1 : 0;
}

// rec[member][set][block] = {Nloc, Ploc, has a tail, Nloc at the last tail, positives behind it}
// A = int64_t (unweighted) or double (weighted).  grid (blocks, members of the batch).
template <typename A>
__global__ __launch_bounds__(kRankThreads) void bank_rank_block_kernel(
    int64_t n, int64_t nb, int U, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ srow,
    const uint8_t* __restrict__ meta, const double* __restrict__ weight,
    const uint32_t* __restrict__ sets /* members x U */, A* __restrict__ rec) {
    __shared__ uint8_t s_meta[kRankBlock];
    __shared__ double s_w[kRankBlock];
    const int fm = blockIdx.y, u = threadIdx.x;
    const int len = rank_stage_dev<A>(n, (int64_t)blockIdx.x * kRankBlock, skey + (size_t)fm * n,
                                      srow + (size_t)fm * n, meta + (size_t)fm * n, weight, s_meta,
                                      s_w);
    if (u >= U) return;
    const uint32_t mask = sets[(size_t)fm * U + u];
    A nloc = 0, ploc = 0, nst = 0, prun = 0, any = 0;
    for (int j = 0; j < len; ++j) {
        const int m = s_meta[j];
        const A w = rank_weight_dev<A>(mask, m, s_w, j);
        if (m & 1) {
            prun += w;
            ploc += w;
        } else {
            nloc += w;
        }
        if (m & 0x80) {
            nst = nloc;
            prun = 0;
            any = 1;
        }
    }
    A* o = rec + (((size_t)fm * U + u) * nb + blockIdx.x) * kRankRec;
    o[0] = nloc;
    o[1] = ploc;
    o[2] = any;
    o[3] = nst;
    o[4] = prun;
}

// One thread per (member, set).  phase 0: the blocks in order, each record replaced by
// {Nin, Nst, Prun} entering the block; res[.][1] = W_pos, res[.][2] = W_neg.  phase 1: res[.][0] =
// the blocks' S_b (record slot 3, bank_rank_finish_kernel) added in block order.
template <typename A>
__global__ __launch_bounds__(kBlock) void bank_rank_carry_kernel(int64_t nb, int cells, int phase,
                                                                 A* __restrict__ rec,
                                                                 A* __restrict__ res /* cells x 3 */) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= cells) return;
    A* r = rec + (size_t)c * nb * kRankRec;
    if (phase == 1) {
        A s = 0;
        for (int64_t b = 0; b < nb; ++b) s += r[b * kRankRec + 3];
        res[(size_t)c * 3] = s;
        return;
    }
    A nin = 0, nst = 0, prun = 0, wpos = 0;
    for (int64_t b = 0; b < nb; ++b, r += kRankRec) {
        const A nloc = r[0], ploc = r[1], any = r[2], lst = r[3], lrun = r[4];
        r[0] = nin;
        r[1] = nst;
        r[2] = prun;
        if (any != 0) {
            nst = nin + lst;
            prun = lrun;
        } else {
            prun += lrun;
        }
        nin += nloc;
        wpos += ploc;
    }
    res[(size_t)c * 3 + 1] = wpos;
    res[(size_t)c * 3 + 2] = nin;
}

// the walk with the carry: record slot 3 = S_b, the block's tails in position order from zero
template <typename A>
__global__ __launch_bounds__(kRankThreads) void bank_rank_finish_kernel(
    int64_t n, int64_t nb, int U, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ srow,
    const uint8_t* __restrict__ meta, const double* __restrict__ weight,
    const uint32_t* __restrict__ sets, A* __restrict__ rec) {
    __shared__ uint8_t s_meta[kRankBlock];
    __shared__ double s_w[kRankBlock];
    const int fm = blockIdx.y, u = threadIdx.x;
    const int len = rank_stage_dev<A>(n, (int64_t)blockIdx.x * kRankBlock, skey + (size_t)fm * n,
                                      srow + (size_t)fm * n, meta + (size_t)fm * n, weight, s_meta,
                                      s_w);
    if (u >= U) return;
    const uint32_t mask = sets[(size_t)fm * U + u];
    A* o = rec + (((size_t)fm * U + u) * nb + blockIdx.x) * kRankRec;
    const A nin = o[0];
    A nst = o[1], prun = o[2], nloc = 0, s = 0;
    for (int j = 0; j < len; ++j) {
        const int m = s_meta[j];
        const A w = rank_weight_dev<A>(mask, m, s_w, j);
        if (m & 1)
            prun += w;
        else
            nloc += w;
        if (m & 0x80) {
            const A ninc = nin + nloc;
            s += prun * (nst + ninc);
            nst = ninc;
            prun = 0;
        }
    }
    o[3] = s;
}

}  // namespace spfm
