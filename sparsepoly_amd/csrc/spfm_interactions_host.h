// spfm_interactions_host.h -- the pure-host helpers of the pair and triple passes (no HIP, no
// engine): the bin choice of one radix-select level, the final order of the top-K candidates and
// the two key formats (pair: feature ids, split at bit 32; triple: compacted ids, looked up).
// Kept apart so that a stand-alone program can run them under a host sanitizer
// (tools/check_interactions_host.cpp).  See DESIGN.md sections 14 and 14a.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace spfm {

constexpr int kInt3KeyBits = 21;  // = kInt3IdBits (spfm_interactions3.hip.h)

// One level of the radix select: hist[0 .. nbins) counts the candidates of the level by bin,
// `above` candidates lie in higher prefixes.  Walks the bins from the top; returns the bin whose
// tail first holds K (-1: fewer than K in all), *tail = above + the counts from that bin up,
// *above_next = the candidates strictly above that bin.
inline int int_select_bin(const uint64_t* hist, int nbins, int64_t above, int64_t K, int64_t* tail,
                          int64_t* above_next) {
    int64_t cum = 0;
    int b = nbins - 1;
    for (; b >= 0; --b) {
        cum += (int64_t)hist[b];
        if (above + cum >= K) break;
    }
    *tail = above + cum;
    *above_next = (b < 0) ? above + cum : above + cum - (int64_t)hist[b];
    return b;
}

// idx[0 .. nk) = the nk = min(K, n) candidates of largest |val|, ties by key ascending (either key
// orders its ids lexicographically); returns nk
inline int64_t int_order_candidates(const std::vector<uint64_t>& keys,
                                    const std::vector<double>& vals, int64_t K,
                                    std::vector<int64_t>& idx) {
    const int64_t n = (int64_t)keys.size();
    idx.resize((size_t)n);
    for (int64_t q = 0; q < n; ++q) idx[(size_t)q] = q;
    const int64_t nk = std::max<int64_t>(0, std::min<int64_t>(K, n));
    std::partial_sort(idx.begin(), idx.begin() + nk, idx.end(), [&](int64_t x, int64_t y) {
        const double ax = std::fabs(vals[(size_t)x]), ay = std::fabs(vals[(size_t)y]);
        if (ax != ay) return ax > ay;
        return keys[(size_t)x] < keys[(size_t)y];
    });
    return nk;
}

// pair key = row id << 32 | column id in feature ids: each half comes back with its 32 bits
inline void int_split_key(uint64_t key, int32_t* row, int32_t* col) {
    *row = (int32_t)(uint32_t)(key >> 32);
    *col = (int32_t)(uint32_t)(key & 0xffffffffu);
}

// triple key = a << 42 | j << 21 | l in compacted ids; returns false when an id is not below `da`
inline bool int3_unpack_key(uint64_t key, const int32_t* ids, int64_t da, int32_t* i, int32_t* j,
                            int32_t* l) {
    const uint64_t mask = (1ull << kInt3KeyBits) - 1ull;
    const uint64_t a = key >> (2 * kInt3KeyBits), b = (key >> kInt3KeyBits) & mask, c = key & mask;
    if (da < 0 || a >= (uint64_t)da || b >= (uint64_t)da || c >= (uint64_t)da) return false;
    *i = ids[a];
    *j = ids[b];
    *l = ids[c];
    return true;
}

}  // namespace spfm
