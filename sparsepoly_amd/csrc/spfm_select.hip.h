// spfm_select.hip.h -- the K best entries of every row of a product that is walked in 64 x 64
// f64 MFMA tiles (spfm_interactions.hip.h), kept in LDS while the tiles stream by.  The one
// selection core of rank_tile_kernel<RANK_SELECT> (spfm_rank.hip.h) and
// part_tile_kernel<PART_SELECT> (spfm_partners.hip.h).  Part of the gfx950 device code of the
// sparse-FM proximal CD core; see DESIGN.md section 15.
//
// Workgroup (strip, ti) owns the 64-row tile ti against the candidate tiles of its strip, in
// ascending order.  What differs between the users comes in as parameters:
//   key     the order key of a stored value (ranker: the score itself; partners: |W|, W or -W)
//   floor   the first `thr` and the value of a short list's padding.  Every admissible key is
//           > floor (ranker: -inf; partners: 0), which keeps the merge's binary search monotone
//   admit   (ra, cb, r, value&) -> whether that accumulator element may enter at all (range
//           checks, exclusion bit, diagonal mask), and the value to store
//   id map  of the merge (strip list id -> output id), and the optional per-row count
//
// Per row, in LDS: `thr`, the key of the K-th best entry seen so far, and a buffer of `cap` =
// K_max + 64 (value, strip-local candidate) entries, 10 bytes each.  A value survives when its
// key is > thr (candidates come in ascending order, so a tie with the K-th loses under the tie
// rule).  Per tile (sel_tile): the survivors of every row are counted (integer LDS counters); a
// row whose buffer could not take them is compacted first -- that raises its thr, and K + 64 <=
// cap always fits afterwards --; then the survivors of the current thr are appended.
// sel_compact, by one wave: every entry is ranked by counting the entries that beat it (key
// descending, candidate ascending: a total order, so the outcome does not depend on the order of
// the appends; the entries travel through lane broadcasts, not LDS), the K best move to their
// rank, thr becomes the K-th key.  A compaction thus absorbs up to cap - K survivors.  At the end
// of the strip (sel_write) every row is compacted and its sorted list written out.
// sel_merge, one wave per row: an entry's final rank is its position in its own strip's list plus,
// by binary search, the entries of every other list that beat it; ranks below K are written.  No
// result bit depends on the partition.  No float atomics.
#pragma once
#include <algorithm>

#include "spfm_interactions.hip.h"

namespace spfm {

constexpr int kSelMaxK = 128;                   // SPFM_RANK_MAX_K, SPFM_INTERACTION_MAX_K
constexpr int kSelCap = kSelMaxK + kIntTile;    // buffer entries per row: K + one tile's worth
constexpr int kSelMaxStrip = 65536;             // candidates per strip: 16-bit local ids
constexpr int64_t kSelSlabDefault = 4096;       // rows per slab
static_assert(kSelCap <= 3 * kWave, "sel_compact keeps three entries per lane");

struct SelLists {
    int K, cap;     // list length; buffer entries per row
    double* lval;   // (n_strips, rows_pad, K) stored values, sorted; padding = floor
    int32_t* lidx;  //                         candidates, INT32_MAX = padding
    double* oval;   // merged (nrow, K)
    int32_t* oidx;
};

// the selection's part of the dynamic LDS, behind the two staging tiles
struct SelLds {
    double* bval;    // [64][cap]
    double* thr;     // [64]
    uint16_t* bidx;  // [64][cap]
    int* cnt;        // [64]
    int* add;        // [64] survivors of the tile
    int cap;
    __device__ SelLds(double* base, int cap_)
        : bval(base),
          thr(bval + (size_t)kIntTile * cap_),
          bidx(reinterpret_cast<uint16_t*>(thr + kIntTile)),
          cnt(reinterpret_cast<int*>(bidx + (size_t)kIntTile * cap_)),
          add(cnt + kIntTile),
          cap(cap_) {}
    __device__ void* end() const { return add + kIntTile; }
};

static inline size_t sel_lds_bytes(int cap) {
    return (size_t)kIntTile * cap * (sizeof(double) + sizeof(uint16_t)) +
           kIntTile * (sizeof(double) + 2 * sizeof(int));
}

// Host: the partition of a selection or count pass over `rows` rows and Tc candidate tiles.
// Slab: the option (0: the default) in whole tiles, at most the rows.  Strip: the option in whole
// tiles, else about 512 workgroups per slab, 16 .. 1024 tiles (a longer strip has fewer
// survivors per candidate: about K ln(strip / K) per row and strip).
struct SelPlan {
    int64_t slab;
    int strip_tiles, n_strips;
    size_t lds;  // dynamic LDS of the selection
};
static inline SelPlan sel_plan(int64_t row_slab, int64_t cand_strip, int64_t rows, int Tc) {
    const auto tiles = [](int64_t v) { return (v + kIntTile - 1) / kIntTile; };
    SelPlan p;
    p.slab = kIntTile * std::min(tiles(row_slab > 0 ? row_slab : kSelSlabDefault), tiles(rows));
    int64_t t = std::min<int64_t>(1024, std::max<int64_t>(16, Tc * (p.slab / kIntTile) / 512));
    if (cand_strip > 0) t = tiles(cand_strip);
    p.strip_tiles = (int)std::min<int64_t>(t, std::min<int64_t>(Tc, kSelMaxStrip / kIntTile));
    p.n_strips = (Tc + p.strip_tiles - 1) / p.strip_tiles;
    p.lds = int_stage_lds_bytes() + sel_lds_bytes(kSelCap);
    return p;
}

// (key descending, candidate ascending)
__device__ __forceinline__ bool rank_beats(double va, unsigned ca, double vb, unsigned cb) {
    return va > vb || (va == vb && ca < cb);
}

__device__ __forceinline__ void sel_init(SelLds s, double floor) {
    if (threadIdx.x < kIntTile) {
        s.thr[threadIdx.x] = floor;
        s.cnt[threadIdx.x] = 0;
        s.add[threadIdx.x] = 0;
    }
}

// One wave: the n entries of row rl's buffer -> its min(n, K) best by key, sorted, at the front
template <typename KeyFn>
__device__ __forceinline__ void sel_compact(SelLds s, int rl, int K, KeyFn key) {
    double* bv = s.bval + (size_t)rl * s.cap;
    uint16_t* bc = s.bidx + (size_t)rl * s.cap;
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(s.cnt[rl]);  // wave-uniform
    double w[3], v[3];
    unsigned c[3];
    int rk[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int i = lane + q * kWave;
        w[q] = i < n ? bv[i] : 0.0;
        v[q] = key(w[q]);
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
            if (rk[q] == K - 1) s.thr[rl] = v[q];
        }
    }
    if (lane == 0) s.cnt[rl] = n < K ? n : K;
    __builtin_amdgcn_wave_barrier();
}

// The accumulators of one tile into the buffers.  loc0: strip-local id of the tile's first
// candidate.  C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15
template <typename AdmitFn, typename KeyFn>
__device__ __forceinline__ void sel_tile(SelLds s, int K, int loc0, AdmitFn admit,
                                         KeyFn key) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    // pass 0: count the survivors; pass 1: append
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int ra = 0; ra < 2; ++ra)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rl = wr * 32 + ra * 16 + l4 + 4 * r;
                    double w;
                    if (admit(ra, cb, r, w) && key(w) > s.thr[rl]) {
                        if (pass == 0) {
                            atomicAdd(&s.add[rl], 1);
                        } else {
                            const int pos = atomicAdd(&s.cnt[rl], 1);  // < cap
                            s.bval[(size_t)rl * s.cap + pos] = w;
                            s.bidx[(size_t)rl * s.cap + pos] =
                                (uint16_t)(loc0 + wc * 32 + cb * 16 + l15);
                        }
                    }
                }
        if (pass == 0) {
            // a row that cannot take its survivors is compacted first: thr rises, and
            // K + 64 <= cap entries always fit afterwards
            __syncthreads();
            for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
                if (s.cnt[rl] + s.add[rl] > s.cap) sel_compact(s, rl, K, key);
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) s.add[rl] = 0;
            }
            __syncthreads();
        }
    }
    // (the next tile reads thr / cnt / add behind the barriers of its staging step)
}

// End of the strip: the sorted list of every row [row0, row0 + 64) < nrow of the slab.
// c0: the strip's first candidate
template <typename KeyFn>
__device__ __forceinline__ void sel_write(SelLds s, const SelLists& o, int strip, int row0,
                                          int nrow, int rows_pad, int c0, double floor,
                                          KeyFn key) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    for (int rl = wave; rl < kIntTile; rl += kBlock / kWave) {
        const int row = row0 + rl;
        if (row >= nrow) continue;  // wave-uniform
        sel_compact(s, rl, o.K, key);
        const int n = s.cnt[rl];
        const size_t at = ((size_t)strip * rows_pad + row) * o.K;
        for (int q = lane; q < o.K; q += kWave) {
            o.lval[at + q] = q < n ? s.bval[(size_t)rl * s.cap + q] : floor;
            o.lidx[at + q] = q < n ? c0 + (int)s.bidx[(size_t)rl * s.cap + q] : INT32_MAX;
        }
    }
}

// One wave per row of the slab: the n_strips lists of the row -> its K best.  id(c): the id that
// is written for list id c.  ocnt (may be NULL): the number of entries written, per row
template <typename KeyFn, typename IdFn>
__device__ __forceinline__ void sel_merge(const SelLists& o, int n_strips, int nrow, int rows_pad,
                                          KeyFn key, IdFn id, int32_t* ocnt) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (row >= nrow) return;  // wave-uniform
    const int K = o.K, N = n_strips * K;
    const size_t sstride = (size_t)rows_pad * K;
    const double* lv = o.lval + (size_t)row * K;
    const int32_t* li = o.lidx + (size_t)row * K;
    int found = 0;
    for (int e = lane; e < N; e += kWave) {
        const int i = e / K, q = e - i * K;
        const double w = lv[i * sstride + q];
        const int32_t c = li[i * sstride + q];
        if (c == INT32_MAX) continue;  // padding of a short list
        ++found;
        const double v = key(w);
        int rank = q;
        for (int j = 0; j < n_strips; ++j) {
            if (j == i) continue;
            const double* jv = lv + j * sstride;
            const int32_t* jc = li + j * sstride;
            int lo = 0, hi = K;  // first entry of list j that does not beat (v, c)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rank_beats(key(jv[mid]), (unsigned)jc[mid], v, (unsigned)c))
                    lo = mid + 1;
                else
                    hi = mid;
            }
            rank += lo;
        }
        if (rank < K) {
            o.oval[(size_t)row * K + rank] = w;
            o.oidx[(size_t)row * K + rank] = id(c);
        }
    }
    if (ocnt != nullptr) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) found += __shfl_xor(found, m, kWave);
        if (lane == 0) ocnt[row] = found < K ? found : K;
    }
}

}  // namespace spfm
