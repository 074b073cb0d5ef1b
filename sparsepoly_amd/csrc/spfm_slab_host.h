// spfm_slab_host.h -- the partition rule of the row-wise read-only units (no HIP, no engine):
// explain and pairs cut a call's rows into slabs, the banks too, fold-in cuts its target columns
// into groups.  Kept apart so that a stand-alone program can run it under a host sanitizer
// (tools/check_slab_host.cpp).  See DESIGN.md section 6.
#pragma once
#include <cstdint>

namespace spfm {

constexpr int64_t kSlabNoCap = INT64_MAX;

// One bound of a slab: `ptr` (n + 1 cumulative offsets: stored entries, pairs, design rows) and
// how much of it a slab may hold.  ptr == nullptr: no such bound.
struct SlabBound {
    const int64_t* ptr;
    int64_t cap;
    bool fits(int64_t r0, int64_t r1) const { return !ptr || ptr[r1] - ptr[r0] <= cap; }
};

// The slab that starts at row r0 < n ends before the returned r1: as many whole rows as fit the
// row cap and both bounds, i.e. the largest r1 in (r0, n] with r1 - r0 <= row_cap that fits --
// and at least one row, even if that row alone breaks a bound.
inline int64_t slab_end(int64_t r0, int64_t n, int64_t row_cap, SlabBound a,
                        SlabBound b = {nullptr, 0}) {
    int64_t r1 = r0 + 1;
    while (r1 < n && r1 - r0 < row_cap && a.fits(r0, r1 + 1) && b.fits(r0, r1 + 1)) ++r1;
    return r1;
}

}  // namespace spfm
