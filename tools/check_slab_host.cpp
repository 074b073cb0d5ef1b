// Stand-alone check of the partition rule of the row-wise read-only units
// (sparsepoly_amd/csrc/spfm_slab_host.h): slab_end against the four loops it replaced, restated
// here as they stood in explain_run / bank_run, pairs_run and foldin_run, and against the rule's
// invariants.  Meant to be built with a host sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/check_slab_host.cpp -o check_slab_host && ./check_slab_host
//
// (tests/test_slab_host.py does that.)
// Prints "ok" and returns 0, or reports the first failed check.
#include <cstdio>
#include <random>
#include <vector>

#include "../sparsepoly_amd/csrc/spfm_slab_host.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

using namespace spfm;
using Cuts = std::vector<int64_t>;

static int64_t row_pairs(const int64_t* indptr, int64_t i) {
    const int64_t m = indptr[i + 1] - indptr[i];
    return m * (m - 1) / 2;
}

// explain_run and bank_run: the entry bound and the row cap
static Cuts old_rows(int64_t n, const int64_t* indptr, int64_t row_cap, int64_t slab_nnz) {
    Cuts cut{0};
    for (int64_t r0 = 0; r0 < n;) {
        int64_t r1 = r0 + 1;
        while (r1 < n && r1 - r0 < row_cap && indptr[r1 + 1] - indptr[r0] <= slab_nnz) ++r1;
        cut.push_back(r1);
        r0 = r1;
    }
    return cut;
}

// pairs_run: and the pair bound, the pairs counted row by row
static Cuts old_pairs(int64_t n, const int64_t* indptr, int64_t row_cap, int64_t slab_nnz,
                      int64_t slab_pairs) {
    Cuts cut{0};
    for (int64_t r0 = 0; r0 < n;) {
        int64_t r1 = r0 + 1, nq = row_pairs(indptr, r0);
        while (r1 < n && r1 - r0 < row_cap && indptr[r1 + 1] - indptr[r0] <= slab_nnz &&
               nq + row_pairs(indptr, r1) <= slab_pairs) {
            nq += row_pairs(indptr, r1);
            ++r1;
        }
        cut.push_back(r1);
        r0 = r1;
    }
    return cut;
}

// foldin_run: columns bounded by the rows of their design matrix, no cap on their number
static Cuts old_columns(int64_t n_cols, const std::vector<int64_t>& cptr, int64_t cap) {
    Cuts cut{0};
    for (int64_t c0 = 0; c0 < n_cols;) {
        int64_t c1 = c0 + 1;
        while (c1 < n_cols && cptr[(size_t)c1 + 1] - cptr[(size_t)c0] <= cap) ++c1;
        cut.push_back(c1);
        c0 = c1;
    }
    return cut;
}

static Cuts new_cuts(int64_t n, int64_t row_cap, SlabBound a, SlabBound b = {nullptr, 0}) {
    Cuts cut{0};
    for (int64_t r0 = 0; r0 < n;) cut.push_back(r0 = slab_end(r0, n, row_cap, a, b));
    return cut;
}

// the cuts strictly increase and cover [0, n); every slab of more than one row meets every
// bound; no slab could take its next row without breaking one
static bool invariants(const Cuts& cut, int64_t n, int64_t row_cap, SlabBound a, SlabBound b) {
    if (cut.empty() || cut.front() != 0 || cut.back() != n) return false;
    for (size_t s = 0; s + 1 < cut.size(); ++s) {
        const int64_t r0 = cut[s], r1 = cut[s + 1];
        if (r1 <= r0) return false;
        if (r1 - r0 > 1 && !(r1 - r0 <= row_cap && a.fits(r0, r1) && b.fits(r0, r1))) return false;
        if (r1 < n && r1 - r0 < row_cap && a.fits(r0, r1 + 1) && b.fits(r0, r1 + 1)) return false;
    }
    return true;
}

// one matrix (row lengths) under one set of caps: all four forms
static int check_case(const std::vector<int64_t>& len, int64_t row_cap, int64_t cap,
                      int64_t pair_cap) {
    const int64_t n = (int64_t)len.size();
    std::vector<int64_t> ptr((size_t)n + 1, 0), pp((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        ptr[(size_t)i + 1] = ptr[(size_t)i] + len[(size_t)i];
        pp[(size_t)i + 1] = pp[(size_t)i] + len[(size_t)i] * (len[(size_t)i] - 1) / 2;
    }
    const SlabBound a = {ptr.data(), cap}, b = {pp.data(), pair_cap}, none = {nullptr, 0};
    const Cuts rows = new_cuts(n, row_cap, a);
    CHECK(rows == old_rows(n, ptr.data(), row_cap, cap));
    CHECK(invariants(rows, n, row_cap, a, none));
    const Cuts pairs = new_cuts(n, row_cap, a, b);
    CHECK(pairs == old_pairs(n, ptr.data(), row_cap, cap, pair_cap));
    CHECK(invariants(pairs, n, row_cap, a, b));
    const Cuts cols = new_cuts(n, kSlabNoCap, a);
    CHECK(cols == old_columns(n, ptr, cap));
    CHECK(invariants(cols, n, kSlabNoCap, a, none));
    return 0;
}

int main() {
    CHECK(new_cuts(0, 1, {nullptr, 0}) == Cuts{0});  // n = 0: no slab
    if (check_case({}, 1, 1, 1)) return 1;
    if (check_case({0}, 1, 1, 1)) return 1;  // one empty row
    for (int64_t cap : {1, 3, 6, 7, 100})
        for (int64_t row_cap : {(int64_t)1, (int64_t)2, kSlabNoCap})
            for (int64_t pair_cap : {1, 3, 21})
                if (check_case({0, 3, 0, 7, 1}, row_cap, cap, pair_cap)) return 1;
    // the cuts themselves, once: entries <= 6 and at most 2 rows; pairs <= 3 on top of that
    {
        const int64_t ptr[] = {0, 0, 3, 3, 10, 11}, pp[] = {0, 0, 3, 3, 24, 24};
        CHECK(new_cuts(5, 2, {ptr, 6}) == (Cuts{0, 2, 3, 4, 5}));
        CHECK(new_cuts(5, kSlabNoCap, {ptr, 6}) == (Cuts{0, 3, 4, 5}));
        CHECK(new_cuts(5, kSlabNoCap, {ptr, 100}, {pp, 3}) == (Cuts{0, 3, 4, 5}));
        CHECK(new_cuts(5, kSlabNoCap, {ptr, 100}, {pp, 21}) == (Cuts{0, 3, 5}));
    }
    std::mt19937_64 rng(11);
    for (int round = 0; round < 1000; ++round) {
        std::vector<int64_t> len((size_t)(rng() % 60));
        for (int64_t& l : len) l = (int64_t)(rng() % 41);
        const int64_t row_cap = (rng() % 4 == 0) ? kSlabNoCap : 1 + (int64_t)(rng() % 200);
        if (check_case(len, row_cap, 1 + (int64_t)(rng() % 200), 1 + (int64_t)(rng() % 200)))
            return 1;
    }
    std::puts("ok");
    return 0;
}
