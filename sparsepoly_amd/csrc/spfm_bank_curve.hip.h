// spfm_bank_curve.hip.h -- average precision, the best F1 and the KS distance of every member of a
// bank on sets of rows (spfm_bank_group_curve).  Part of the gfx950 device
// code, beside spfm_bank_rank.hip.h: it reads that file's member-major images (key, meta, weight)
// and the sorted copies skey / srow of a batch, and leaves its kernels untouched.
//
// Layout.  As in spfm_bank_rank.hip.h: position p of member f holds the p-th smallest score and
// its row, equal scores in row order.  This walk goes from the top down: q = n - 1 - p, block b is
// the positions q in [kRankBlock b, kRankBlock b + kRankBlock).  Going down a tie run ends at its
// ascending head: p == 0 or skey[p - 1] != skey[p], read from memory (so the last position of a
// block looks into the next block).
//
// The statistics.  For one member and one set, with w_p the weight of the row at position p where
// that row is in the set and 0 where it is not (1 / 0 unweighted), and the runs r from the top down:
//   Prun(r), Nrun(r) = the weights of the positives / negatives of run r,
//   TP(r), FP(r)     = the weights of the positives / negatives of all runs down to and including r,
//   r is a candidate when Prun(r) + Nrun(r) > 0,
//   AP   = (1 / W_pos) sum over the candidates of  Prun(r) * (TP(r) / (TP(r) + FP(r))),
//   F1   = max over the candidates of  2 TP(r) / ((TP(r) + FP(r)) + W_pos),
//   KS   = max over the candidates of  | TP(r) / W_pos - FP(r) / W_neg |,
// each maximum with its TP, FP and the position of its run's head (the host reads the score there).
// Of several candidates that reach a maximum the one met first -- the highest score -- is kept: a
// later one replaces it only when strictly greater.  Unweighted (A = int64_t) the two comparisons
// are exact: F1 by TP_a (TP_b + FP_b + n_pos) > TP_b (TP_a + FP_a + n_pos) in unsigned 64 bit
// (n < 2^31: every product is below 2^63), KS by |TP n_neg - FP n_pos| in int64 (below 2^62).
// Weighted (A = double) the quotients above are compared as written: IEEE operations, the build has
// -ffp-contract=off and no fast-math.  Every addend anywhere is non-negative.
//
// Work split.  One workgroup of one wavefront per (block, member of the batch).  The wave stages
// its block's bytes (meta | head << 7) and weights in LDS (curve_stage_dev); then lane u < U is set
// u and walks the block's positions one after the other, its state in scalars.  All lanes read the
// same LDS address (a broadcast); the per-set state is never an array.  Launches per batch:
//   bank_curve_block_kernel   per block, from zero: P, N (the block's positives / negatives),
//                             whether a run ends in it, Prun / Nrun of the stretch behind its last
//                             run end (of the whole block where none ends);
//   bank_curve_carry_kernel   phase 0, one thread per (member, set), the blocks in top-down order:
//                             replaces each block's record by what enters the block -- TPin, FPin
//                             and Prun / Nrun of the run that is open at its start -- and gives
//                             W_pos, W_neg;
//   bank_curve_finish_kernel  per block: the walk again with the carry; the block's AP partial sum
//                             from zero, its best F1 candidate and its best KS candidate;
//   bank_curve_carry_kernel   phase 1: adds the AP partials in block order, reduces the blocks'
//                             bests in block order (strictly greater replaces) and reads the keys
//                             at the two winning positions.
//
// Summation order (a function of the sorted position alone; weighted and unweighted alike).
//   ploc(q)   = ((0 + w_b0) + w_b1) + ...        positives of q's block down to q, in walk order;
//   TPin(b)   = ((0 + P_0) + P_1) + ...          the blocks before b, in block order;
//   TP(r)     = TPin(b) + ploc(end of r);  FP(r) likewise from the negatives;
//   Prun(r)   = ((c + w_r0) + w_r1) + ...        the run's positives in walk order, where c is 0 for
//               a run that starts in r's block and else Prun carried into the block: the sum, block
//               after block in block order, of the positives ((0 + w) + w) ... of the run's stretch
//               in each earlier block;  Nrun(r) likewise;
//   AP_b      = ((0 + T_r0) + T_r1) + ...        T_r = (double)Prun(r) * ((double)TP(r) /
//               (double)(TP(r) + FP(r))), the candidates that end in block b in walk order;
//   AP sum    = ((0 + AP_0) + AP_1) + ...  in block order;   the host divides by W_pos once;
//   W_pos     = TPin(last) + P_last,  W_neg = FPin(last) + N_last: the very values TP and FP take at
//               the last run end.
// Nothing depends on the slabs, on F, on the member's position or on the batch; a row of weight 0
// adds exact zeros and a run of such rows is no candidate.  No atomics.
#pragma once
#include "spfm_bank_rank.hip.h"

namespace spfm {

// One (member, set, block) record, 8-byte fields.  After bank_curve_block_kernel: tp, fp = P, N of
// the block, prun, nrun = the stretch behind its last run end, any.  After phase 0 of the carry:
// tp, fp = TPin, FPin, prun, nrun = the run open at the block's start.  The finish kernel fills the
// rest; a position of -1 says that no candidate ends in the block.
template <typename A>
struct CurveRec {
    A tp, fp, prun, nrun;
    int64_t any;
    double ap;
    A f1_tp, f1_fp;
    int64_t f1_pos;
    A ks_tp, ks_fp;
    int64_t ks_pos;
};
constexpr int kCurveRec = 12;  // 8-byte values per record
static_assert(sizeof(CurveRec<int64_t>) == 8 * kCurveRec && sizeof(CurveRec<double>) == 8 * kCurveRec,
              "the record is kCurveRec values of 8 bytes in both instantiations");

// One (member, set) result.  f1_pos / ks_pos: the ascending position p of the winning run's head,
// -1 where the set has no candidate; f1_key / ks_key: skey there.
template <typename A>
struct CurveRes {
    A wpos, wneg;
    double ap;  // the sum of the terms: not yet divided by W_pos
    A f1_tp, f1_fp;
    int64_t f1_pos;
    uint64_t f1_key;
    A ks_tp, ks_fp;
    int64_t ks_pos;
    uint64_t ks_key;
};
constexpr int kCurveRes = 11;  // 8-byte values per result
static_assert(sizeof(CurveRes<int64_t>) == 8 * kCurveRes && sizeof(CurveRes<double>) == 8 * kCurveRes,
              "the result is kCurveRes values of 8 bytes in both instantiations");

// the block's positions, top down, into LDS: s_meta[j] = meta of the row | head << 7, s_w[j] its
// weight; j = 0 is the position q0 from the top, p = n - 1 - q0 - j ascending
template <typename A>
__device__ __forceinline__ int curve_stage_dev(int64_t n, int64_t q0, const uint64_t* __restrict__ skey,
                                               const uint32_t* __restrict__ srow,
                                               const uint8_t* __restrict__ meta,
                                               const double* __restrict__ weight, uint8_t* s_meta,
                                               double* s_w) {
    const int len = (int)min((int64_t)kRankBlock, n - q0);
    for (int j = threadIdx.x; j < len; j += kRankThreads) {
        const int64_t p = n - 1 - q0 - j;
        const uint32_t r = srow[p];
        const bool head = p == 0 || skey[p - 1] != skey[p];
        s_meta[j] = (uint8_t)(meta[r] | (head ? 0x80 : 0));
        if constexpr (std::is_same<A, double>::value) s_w[j] = weight[r];
    }
    __syncthreads();
    return len;
}

// is the F1 of (tp, fp) strictly greater than that of (btp, bfp)?
template <typename A>
__device__ __forceinline__ bool curve_f1_greater_dev(A tp, A fp, A btp, A bfp, A wpos) {
    if constexpr (std::is_same<A, double>::value)
        return 2.0 * tp / ((tp + fp) + wpos) > 2.0 * btp / ((btp + bfp) + wpos);
    else
        return (uint64_t)tp * (uint64_t)(btp + bfp + wpos) > (uint64_t)btp * (uint64_t)(tp + fp + wpos);
}

// what the KS comparison goes by: |TP / W_pos - FP / W_neg|, unweighted times n_pos n_neg
template <typename A>
__device__ __forceinline__ A curve_ks_dev(A tp, A fp, A wpos, A wneg) {
    if constexpr (std::is_same<A, double>::value) {
        return fabs(tp / wpos - fp / wneg);
    } else {
        const int64_t v = tp * wneg - fp * wpos;
        return v < 0 ? -v : v;
    }
}

// rec[member][set][block] = {P, N, Prun, Nrun behind the last run end, any}
// A = int64_t (unweighted) or double (weighted).  grid (blocks, members of the batch).
template <typename A>
__global__ __launch_bounds__(kRankThreads) void bank_curve_block_kernel(
    int64_t n, int64_t nb, int U, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ srow,
    const uint8_t* __restrict__ meta, const double* __restrict__ weight,
    const uint32_t* __restrict__ sets /* members x U */, CurveRec<A>* __restrict__ rec) {
    __shared__ uint8_t s_meta[kRankBlock];
    __shared__ double s_w[kRankBlock];
    const int fm = blockIdx.y, u = threadIdx.x;
    const int len = curve_stage_dev<A>(n, (int64_t)blockIdx.x * kRankBlock, skey + (size_t)fm * n,
                                       srow + (size_t)fm * n, meta + (size_t)fm * n, weight, s_meta,
                                       s_w);
    if (u >= U) return;
    const uint32_t mask = sets[(size_t)fm * U + u];
    A ploc = 0, nloc = 0, prun = 0, nrun = 0;
    int64_t any = 0;
    for (int j = 0; j < len; ++j) {
        const int m = s_meta[j];
        const A w = rank_weight_dev<A>(mask, m, s_w, j);
        if (m & 1) {
            prun += w;
            ploc += w;
        } else {
            nrun += w;
            nloc += w;
        }
        if (m & 0x80) {
            prun = 0;
            nrun = 0;
            any = 1;
        }
    }
    CurveRec<A>* o = rec + ((size_t)fm * U + u) * nb + blockIdx.x;
    o->tp = ploc;
    o->fp = nloc;
    o->prun = prun;
    o->nrun = nrun;
    o->any = any;
}

// One thread per (member, set); cell c is member c / U of the batch.  phase 0: the blocks in
// top-down order, each record replaced by {TPin, FPin, Prun, Nrun} entering the block; res.wpos,
// res.wneg.  phase 1 (after bank_curve_finish_kernel): the AP partials added in block order, the
// blocks' bests reduced in block order, the keys at the winning positions.
template <typename A>
__global__ __launch_bounds__(kBlock) void bank_curve_carry_kernel(
    int64_t n, int64_t nb, int U, int cells, int phase, const uint64_t* __restrict__ skey,
    CurveRec<A>* __restrict__ rec, CurveRes<A>* __restrict__ res) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= cells) return;
    CurveRec<A>* r = rec + (size_t)c * nb;
    CurveRes<A>* o = res + c;
    if (phase == 0) {
        A tpin = 0, fpin = 0, prun = 0, nrun = 0;
        for (int64_t b = 0; b < nb; ++b, ++r) {
            const A p = r->tp, q = r->fp, lp = r->prun, ln = r->nrun;
            const bool any = r->any != 0;
            r->tp = tpin;
            r->fp = fpin;
            r->prun = prun;
            r->nrun = nrun;
            if (any) {
                prun = lp;
                nrun = ln;
            } else {
                prun += lp;
                nrun += ln;
            }
            tpin += p;
            fpin += q;
        }
        o->wpos = tpin;
        o->wneg = fpin;
        return;
    }
    const A wpos = o->wpos, wneg = o->wneg;
    double ap = 0.0;
    A f1_tp = 0, f1_fp = 0, ks_tp = 0, ks_fp = 0, ks_v = 0;
    int64_t f1_pos = -1, ks_pos = -1;
    for (int64_t b = 0; b < nb; ++b, ++r) {
        ap += r->ap;
        if (r->f1_pos < 0) continue;  // no candidate ends in the block
        if (f1_pos < 0 || curve_f1_greater_dev<A>(r->f1_tp, r->f1_fp, f1_tp, f1_fp, wpos)) {
            f1_tp = r->f1_tp;
            f1_fp = r->f1_fp;
            f1_pos = r->f1_pos;
        }
        const A v = curve_ks_dev<A>(r->ks_tp, r->ks_fp, wpos, wneg);
        if (ks_pos < 0 || v > ks_v) {
            ks_tp = r->ks_tp;
            ks_fp = r->ks_fp;
            ks_pos = r->ks_pos;
            ks_v = v;
        }
    }
    const uint64_t* sk = skey + (size_t)(c / U) * n;
    o->ap = ap;
    o->f1_tp = f1_tp;
    o->f1_fp = f1_fp;
    o->f1_pos = f1_pos;
    o->f1_key = f1_pos >= 0 ? sk[f1_pos] : 0;
    o->ks_tp = ks_tp;
    o->ks_fp = ks_fp;
    o->ks_pos = ks_pos;
    o->ks_key = ks_pos >= 0 ? sk[ks_pos] : 0;
}

// the walk with the carry: the block's AP partial from zero and its two best candidates
template <typename A>
__global__ __launch_bounds__(kRankThreads) void bank_curve_finish_kernel(
    int64_t n, int64_t nb, int U, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ srow,
    const uint8_t* __restrict__ meta, const double* __restrict__ weight,
    const uint32_t* __restrict__ sets, CurveRec<A>* __restrict__ rec,
    const CurveRes<A>* __restrict__ res) {
    __shared__ uint8_t s_meta[kRankBlock];
    __shared__ double s_w[kRankBlock];
    const int fm = blockIdx.y, u = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * kRankBlock;
    const int len = curve_stage_dev<A>(n, q0, skey + (size_t)fm * n, srow + (size_t)fm * n,
                                       meta + (size_t)fm * n, weight, s_meta, s_w);
    if (u >= U) return;
    const uint32_t mask = sets[(size_t)fm * U + u];
    CurveRec<A>* o = rec + ((size_t)fm * U + u) * nb + blockIdx.x;
    const A wpos = res[(size_t)fm * U + u].wpos, wneg = res[(size_t)fm * U + u].wneg;
    const A tpin = o->tp, fpin = o->fp;
    A prun = o->prun, nrun = o->nrun, ploc = 0, nloc = 0;
    double ap = 0.0;
    A f1_tp = 0, f1_fp = 0, ks_tp = 0, ks_fp = 0, ks_v = 0;
    int64_t f1_pos = -1, ks_pos = -1;
    for (int j = 0; j < len; ++j) {
        const int m = s_meta[j];
        const A w = rank_weight_dev<A>(mask, m, s_w, j);
        if (m & 1) {
            prun += w;
            ploc += w;
        } else {
            nrun += w;
            nloc += w;
        }
        if (m & 0x80) {
            if (prun + nrun > 0) {  // a candidate: the run holds weight of the set
                const A tp = tpin + ploc, fp = fpin + nloc;
                const int64_t p = n - 1 - q0 - j;
                ap += (double)prun * ((double)tp / (double)(tp + fp));
                if (f1_pos < 0 || curve_f1_greater_dev<A>(tp, fp, f1_tp, f1_fp, wpos)) {
                    f1_tp = tp;
                    f1_fp = fp;
                    f1_pos = p;
                }
                const A v = curve_ks_dev<A>(tp, fp, wpos, wneg);
                if (ks_pos < 0 || v > ks_v) {
                    ks_tp = tp;
                    ks_fp = fp;
                    ks_pos = p;
                    ks_v = v;
                }
            }
            prun = 0;
            nrun = 0;
        }
    }
    o->ap = ap;
    o->f1_tp = f1_tp;
    o->f1_fp = f1_fp;
    o->f1_pos = f1_pos;
    o->ks_tp = ks_tp;
    o->ks_fp = ks_fp;
    o->ks_pos = ks_pos;
}

}  // namespace spfm
