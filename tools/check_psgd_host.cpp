// Stand-alone check of the host rules of the minibatch unit (sparsepoly_amd/csrc/spfm_psgd_host.h)
// against the loops they replaced, restated here as they stood in spfm_engine_psgd.hip, and
// against their invariants.  Meant to be built with a host sanitizer:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/check_psgd_host.cpp -o check_psgd_host && ./check_psgd_host
//
// (tests/test_psgd_host.py does that.)
// Prints "ok" and returns 0, or reports the first failed check.
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../sparsepoly_amd/csrc/spfm_psgd_host.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

using namespace spfm;

// ------------------------------------------------------------------ the loops as they stood
static void old_eta(int lr, double eta0, double alpha, double beta, double power_t, int64_t it,
                    double* eta_P, double* eta_w) {
    if (lr == 0) {
        *eta_P = eta0;
        *eta_w = eta0;
    } else if (lr == 1) {
        const double eta_it = eta0 * (double)it;
        *eta_P = eta0 / std::pow(1.0 + eta_it * beta, power_t);
        *eta_w = eta0 / std::pow(1.0 + eta_it * alpha, power_t);
    } else if (lr == 2) {
        *eta_P = 1.0 / (beta * (double)it);
        *eta_w = 1.0 / (alpha * (double)it);
    } else {
        const double eta = eta0 / std::pow((double)it, power_t);
        *eta_P = eta;
        *eta_w = eta;
    }
}

// psgd_batches_tl, graph route
static std::vector<PsgdBatch> old_tabulate(int lr, double eta0, double alpha, double beta,
                                           double gamma, double power_t, int64_t batch_size,
                                           int64_t n_items, int64_t it) {
    const int64_t nbat = (n_items + batch_size - 1) / batch_size;
    std::vector<PsgdBatch> h_sched((size_t)nbat);
    for (int64_t bi = 0; bi < nbat; ++bi) {
        const int64_t pos = bi * batch_size;
        const int B = (int)std::min<int64_t>(batch_size, n_items - pos);
        double eta_P, eta_w;
        old_eta(lr, eta0, alpha, beta, power_t, it + bi, &eta_P, &eta_w);
        PsgdBatch& e = h_sched[(size_t)bi];
        e.pos = pos;
        e.B = B;
        e.pad = 0;
        e.cp = eta_P / (double)B;
        e.denp = 1.0 + eta_P * beta;
        e.strength = gamma * eta_P / (1 + eta_P * beta);
        e.cw = eta_w / (double)B;
        e.denw = 1 + eta_w * alpha;
    }
    return h_sched;
}

// psgd_epoch, several ranks
static bool old_shard(const int32_t* indices_samples, int64_t n_samples, int64_t row_lo, int64_t n,
                      int64_t batch_size, std::vector<int64_t>& sg_lpos,
                      std::vector<int32_t>& sg_lB, std::vector<int32_t>& sg_gB,
                      std::vector<int32_t>& local) {
    const int64_t nbat = (n_samples + batch_size - 1) / batch_size;
    sg_lpos.assign((size_t)nbat, 0);
    sg_lB.assign((size_t)nbat, 0);
    sg_gB.assign((size_t)nbat, 0);
    local.clear();
    local.reserve((size_t)n);
    for (int64_t bi = 0; bi < nbat; ++bi) {
        const int64_t pos = bi * batch_size;
        const int64_t B = std::min<int64_t>(batch_size, n_samples - pos);
        sg_lpos[(size_t)bi] = (int64_t)local.size();
        for (int64_t q = pos; q < pos + B; ++q) {
            const int64_t i = (int64_t)indices_samples[q] - row_lo;
            if (i >= 0 && i < n) local.push_back((int32_t)i);
        }
        sg_lB[(size_t)bi] = (int32_t)((int64_t)local.size() - sg_lpos[(size_t)bi]);
        sg_gB[(size_t)bi] = (int32_t)B;
    }
    return (int64_t)local.size() == n;
}

// psgd_epoch (indices_samples) and psgd_pairs_sample (order)
static bool old_permutation(const int32_t* order, int64_t m) {
    std::vector<char> seen((size_t)m, 0);
    for (int64_t q = 0; q < m; ++q) {
        const int32_t i = order[q];
        if (i < 0 || i >= m || seen[(size_t)i]) return false;
        seen[(size_t)i] = 1;
    }
    return true;
}

static const char* old_csr_error(int64_t rows, int64_t n_cand, const int64_t* ptr,
                                 const int32_t* idx) {
    if (!ptr || ptr[0] != 0) return "indptr[0] != 0";
    for (int64_t b = 0; b < rows; ++b) {
        if (ptr[b + 1] < ptr[b]) return "indptr not monotone";
        if (ptr[b + 1] > ptr[b] && !idx) return "indices missing";
        for (int64_t e = ptr[b]; e < ptr[b + 1]; ++e) {
            if (idx[e] < 0 || idx[e] >= n_cand) return "a candidate index outside [0, n_cand)";
            if (e > ptr[b] && idx[e] <= idx[e - 1]) return "indices not strictly ascending";
        }
    }
    return nullptr;
}

// psgd_pairs_set_sampler: the merge per row, the messages reduced to (kind, row)
static int old_positives(int64_t n_ctx, int64_t n_cand, const int64_t* pos_ptr,
                         const int32_t* pos_idx, const int64_t* forb_ptr, const int32_t* forb_idx,
                         int64_t* row) {
    for (int64_t b = 0; b < n_ctx; ++b) {
        const int64_t p0 = pos_ptr[b], p1 = pos_ptr[b + 1];
        if (p1 == p0) continue;
        int64_t f = forb_ptr[b];
        const int64_t f1 = forb_ptr[b + 1];
        for (int64_t e = p0; e < p1; ++e) {  // both sorted: one merge
            while (f < f1 && forb_idx[f] < pos_idx[e]) ++f;
            if (f == f1 || forb_idx[f] != pos_idx[e]) {
                *row = b;
                return 1;
            }
        }
        if (f1 - forb_ptr[b] >= n_cand) {
            *row = b;
            return 2;
        }
    }
    return 0;
}

// psgd_pairs_check and psgd_pairs_set_sampler
static int32_t old_shared_column(const std::vector<uint8_t>& side, int32_t d,
                                 const std::vector<int64_t>& h_cptr,
                                 const std::vector<int32_t>& h_cidx) {
    for (int32_t j = 0; j < d; ++j) {
        unsigned both = 0;
        for (int64_t e = h_cptr[(size_t)j]; e < h_cptr[(size_t)j + 1]; ++e)
            both |= side[(size_t)h_cidx[(size_t)e]];
        if (both == 3) return j;
    }
    return -1;
}

// ------------------------------------------------------------------ the checks
static PsgdStep make_step(int lr, double eta0, double alpha, double beta, double gamma,
                          double power_t, int64_t batch_size, int64_t* it) {
    return PsgdStep{2, alpha, beta, gamma, eta0, lr, power_t, batch_size, 1, it};
}

static int check_tabulate(int lr, double eta0, double alpha, double beta, double gamma,
                          double power_t, int64_t batch_size, int64_t n_items, int64_t it0) {
    int64_t it = it0;
    const PsgdStep st = make_step(lr, eta0, alpha, beta, gamma, power_t, batch_size, &it);
    std::vector<PsgdBatch> got(3);  // a stale table of another size
    tabulate_epoch(st, n_items, it0, got);
    const std::vector<PsgdBatch> want =
        old_tabulate(lr, eta0, alpha, beta, gamma, power_t, batch_size, n_items, it0);
    CHECK(got.size() == want.size());
    int64_t next = 0;
    for (size_t b = 0; b < got.size(); ++b) {
        CHECK(std::memcmp(&got[b], &want[b], sizeof(PsgdBatch)) == 0);  // every bit, pad included
        CHECK(got[b].pos == next && got[b].B >= 1 && got[b].B <= batch_size);
        next += got[b].B;
        // the eager route forms the same scalars one minibatch at a time
        const PsgdBatch one = st.batch(it0 + (int64_t)b, got[b].B);
        CHECK(one.cp == want[b].cp && one.denp == want[b].denp && one.cw == want[b].cw &&
              one.strength == want[b].strength && one.denw == want[b].denw);
    }
    CHECK(next == n_items);  // [0, n_items) exactly once
    CHECK(it == it0);        // the table does not advance the counter
    return 0;
}

static int check_shard(const std::vector<int32_t>& order, int64_t row_lo, int64_t n,
                       int64_t batch_size, bool want_ok) {
    const int64_t ng = (int64_t)order.size();
    std::vector<int64_t> lp, lp0;
    std::vector<int32_t> lB, gB, loc, lB0, gB0, loc0;
    const bool ok = shard_batches(order.data(), ng, row_lo, n, batch_size, lp, lB, gB, loc);
    const bool ok0 = old_shard(order.data(), ng, row_lo, n, batch_size, lp0, lB0, gB0, loc0);
    CHECK(ok == ok0 && ok == want_ok);
    CHECK(lp == lp0 && lB == lB0 && gB == gB0 && loc == loc0);
    CHECK(std::accumulate(gB.begin(), gB.end(), (int64_t)0) == ng);
    CHECK(std::accumulate(lB.begin(), lB.end(), (int64_t)0) == (int64_t)loc.size());
    if (ok) CHECK((int64_t)loc.size() == n && is_permutation(loc.data(), n));
    for (size_t b = 0; b < lB.size(); ++b)
        CHECK(lB[b] >= 0 && lB[b] <= gB[b] && lp[b] + lB[b] <= (int64_t)loc.size());
    return 0;
}

struct Csr {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx;
};

// a valid CSR: each row a random ascending subset of [0, n_cand)
static Csr random_csr(std::mt19937_64& rng, int64_t rows, int64_t n_cand, unsigned keep_of_4) {
    Csr c;
    c.ptr.push_back(0);
    for (int64_t b = 0; b < rows; ++b) {
        for (int32_t j = 0; j < n_cand; ++j)
            if (rng() % 4 < keep_of_4) c.idx.push_back(j);
        c.ptr.push_back((int64_t)c.idx.size());
    }
    return c;
}

static int check_csr(int64_t rows, int64_t n_cand, const int64_t* ptr, const int32_t* idx,
                     const char* want) {
    const char* got = sampler_csr_error(rows, n_cand, ptr, idx);
    const char* old = old_csr_error(rows, n_cand, ptr, idx);
    CHECK((got == nullptr) == (old == nullptr));
    CHECK(!got || std::string(got) == old);
    if (want != (const char*)-1) {
        CHECK((got == nullptr) == (want == nullptr));
        CHECK(!got || std::string(got) == want);
    }
    return 0;
}

static int check_positives(int64_t n_cand, const Csr& pos, const Csr& forb, int want_kind,
                           int64_t want_row) {
    const int64_t n_ctx = (int64_t)pos.ptr.size() - 1;
    int64_t row = -1, row0 = -1;
    const int kind = check_positives_in_forbidden(n_ctx, n_cand, pos.ptr.data(), pos.idx.data(),
                                                  forb.ptr.data(), forb.idx.data(), &row);
    const int kind0 = old_positives(n_ctx, n_cand, pos.ptr.data(), pos.idx.data(),
                                    forb.ptr.data(), forb.idx.data(), &row0);
    CHECK(kind == kind0 && (kind == 0 || row == row0));
    if (want_kind >= 0) CHECK(kind == want_kind && (kind == 0 || row == want_row));
    return 0;
}

int main() {
    // ---- tabulate_epoch: the sizes around a run of 32, every learning-rate rule
    for (int64_t n_items : {1, 31, 32, 33, 64, 65})
        for (int64_t batch_size : {(int64_t)1, (int64_t)32, n_items, n_items + 1})
            for (int lr = 0; lr <= 3; ++lr)
                for (int64_t it0 : {1, 1000})
                    if (check_tabulate(lr, 0.05, 0.01, 0.5, 0.003, 0.8, batch_size, n_items, it0))
                        return 1;
    {
        int64_t it = 1;
        PsgdStep st = make_step(1, 0.05, 0.01, 0.5, 0.003, 0.8, 4, &it);
        CHECK(st.check("w").empty());
        st.it = nullptr;
        CHECK(st.check("w") == "w: it is required");
        st.it = &it;
        st.batch_size = 0;
        CHECK(st.check("psgd pairs") == "psgd pairs: batch_size must be >= 1");
        st.batch_size = 1;
        st.lr = 4;
        CHECK(st.check("psgd") == "psgd: learning_rate is not supported.");
        st.lr = -1;
        CHECK(st.check("psgd") == "psgd: learning_rate is not supported.");
        st.lr = 3;
        it = 0;
        CHECK(st.check("psgd") == "psgd: it must be >= 1");
    }
    // ---- shard_batches: 3 ranks over 10 samples (rows [0,3), [3,7), [7,10)), batches of 4
    {
        const std::vector<int32_t> order = {3, 4, 5, 6, 0, 1, 2, 7, 8, 9};
        if (check_shard(order, 0, 3, 4, true)) return 1;  // no share of batches 0 and 2
        if (check_shard(order, 3, 4, 4, true)) return 1;  // all of batch 0, nothing else
        if (check_shard(order, 7, 3, 4, true)) return 1;
        std::vector<int64_t> lp;
        std::vector<int32_t> lB, gB, loc;
        CHECK(shard_batches(order.data(), 10, 0, 3, 4, lp, lB, gB, loc));
        CHECK((lB == std::vector<int32_t>{0, 3, 0}) && (gB == std::vector<int32_t>{4, 4, 2}));
        CHECK((lp == std::vector<int64_t>{0, 0, 3}) && (loc == std::vector<int32_t>{0, 1, 2}));
        const std::vector<int32_t> lacks = {3, 4, 5, 6, 0, 1, 7, 7, 8, 9};  // row 2 is missing
        if (check_shard(lacks, 0, 3, 4, false)) return 1;
        if (check_shard(lacks, 3, 4, 4, true)) return 1;
    }
    // ---- is_permutation
    {
        CHECK(is_permutation(nullptr, 0));
        const int32_t one[] = {0}, rep[] = {0, 2, 2}, neg[] = {0, -1, 2}, hi[] = {0, 3, 1},
                      good[] = {2, 0, 1};
        CHECK(is_permutation(one, 1) && is_permutation(good, 3));
        CHECK(!is_permutation(rep, 3) && !is_permutation(neg, 3) && !is_permutation(hi, 3));
        const int32_t one_bad[] = {1};
        CHECK(!is_permutation(one_bad, 1));
    }
    // ---- the sampler's CSRs: one case per message
    {
        const int64_t ptr[] = {0, 2, 2, 3}, ptr0[] = {1, 2, 2, 3}, down[] = {0, 2, 1, 3};
        const int32_t idx[] = {0, 3, 1}, out_hi[] = {0, 4, 1}, out_lo[] = {-1, 3, 1},
                      same[] = {3, 3, 1}, desc[] = {3, 0, 1};
        if (check_csr(3, 4, ptr, idx, nullptr)) return 1;
        if (check_csr(3, 4, nullptr, idx, "indptr[0] != 0")) return 1;
        if (check_csr(3, 4, ptr0, idx, "indptr[0] != 0")) return 1;
        if (check_csr(3, 4, down, idx, "indptr not monotone")) return 1;
        if (check_csr(3, 4, ptr, nullptr, "indices missing")) return 1;
        if (check_csr(3, 4, ptr, out_hi, "a candidate index outside [0, n_cand)")) return 1;
        if (check_csr(3, 4, ptr, out_lo, "a candidate index outside [0, n_cand)")) return 1;
        if (check_csr(3, 4, ptr, same, "indices not strictly ascending")) return 1;
        if (check_csr(3, 4, ptr, desc, "indices not strictly ascending")) return 1;
        const int64_t empty[] = {0, 0, 0, 0};
        if (check_csr(3, 4, empty, nullptr, nullptr)) return 1;  // no entries: no list needed
    }
    // ---- positives within forbidden, a candidate left free (n_cand = 4)
    {
        const Csr pos = {{0, 1, 1, 3}, {2, 0, 3}};
        if (check_positives(4, pos, pos, 0, -1)) return 1;
        // row 0 forbids n_cand - 1 candidates: accepted; row 1 has no positive and may be full
        if (check_positives(4, pos, {{0, 3, 7, 9}, {0, 2, 3, 0, 1, 2, 3, 0, 3}}, 0, -1)) return 1;
        // row 0 forbids all four: refused
        if (check_positives(4, pos, {{0, 4, 4, 6}, {0, 1, 2, 3, 0, 3}}, kForbidsEveryCandidate, 0))
            return 1;
        // row 2 lacks its positive 3 (the list ends first) / its positive 0 (another stands there)
        if (check_positives(4, pos, {{0, 1, 1, 2}, {2, 0}}, kForbiddenLacksPositive, 2)) return 1;
        if (check_positives(4, pos, {{0, 1, 1, 3}, {2, 1, 3}}, kForbiddenLacksPositive, 2)) return 1;
        // both faults in one row: the missing positive is reported
        if (check_positives(4, {{0, 1}, {0}}, {{0, 4}, {1, 2, 3, 3}}, kForbiddenLacksPositive, 0))
            return 1;
    }
    // ---- the disjoint-column rule
    {
        const std::vector<int64_t> cptr = {0, 2, 2, 4};  // column 0: rows 0, 1; column 2: rows 1, 2
        const std::vector<int32_t> cidx = {0, 1, 1, 2};
        CHECK(first_shared_column({1, 1, 2}, 3, cptr.data(), cidx.data()) == 2);
        CHECK(first_shared_column({1, 2, 2}, 3, cptr.data(), cidx.data()) == 0);
        CHECK(first_shared_column({1, 0, 2}, 3, cptr.data(), cidx.data()) == -1);
        CHECK(first_shared_column({3, 0, 0}, 3, cptr.data(), cidx.data()) == 0);  // both in one row
        CHECK(first_shared_column({1, 2}, 0, cptr.data(), cidx.data()) == -1);
    }
    // ---- 1000 seeded random cases per function against the restated loops
    std::mt19937_64 rng(17);
    for (int round = 0; round < 1000; ++round) {
        const auto unit = [&] { return (double)(rng() % 1000 + 1) / 1000.0; };
        const int64_t n_items = 1 + (int64_t)(rng() % 200);
        if (check_tabulate((int)(rng() % 4), unit(), unit(), unit(), unit(), unit(),
                           1 + (int64_t)(rng() % 70), n_items, 1 + (int64_t)(rng() % 100000)))
            return 1;
        // a sharded epoch: a random order (sometimes with one entry overwritten), a random rank
        const int64_t ng = 1 + (int64_t)(rng() % 60);
        std::vector<int32_t> order((size_t)ng);
        std::iota(order.begin(), order.end(), 0);
        std::shuffle(order.begin(), order.end(), rng);
        const int64_t row_lo = (int64_t)(rng() % (uint64_t)ng);
        const int64_t n = (int64_t)(rng() % (uint64_t)(ng - row_lo + 1));
        CHECK(is_permutation(order.data(), ng) && old_permutation(order.data(), ng));
        if (check_shard(order, row_lo, n, 1 + (int64_t)(rng() % 9), true)) return 1;
        std::vector<int32_t> bad = order;
        bad[(size_t)(rng() % (uint64_t)ng)] = (int32_t)(rng() % (uint64_t)(ng + 2)) - 1;
        const bool perm = old_permutation(bad.data(), ng);
        CHECK(is_permutation(bad.data(), ng) == perm);
        if (!perm) {  // its verdict is whatever the loop gave
            std::vector<int64_t> a, a0;
            std::vector<int32_t> b, c, e, b0, c0, e0;
            CHECK(shard_batches(bad.data(), ng, row_lo, n, 3, a, b, c, e) ==
                  old_shard(bad.data(), ng, row_lo, n, 3, a0, b0, c0, e0));
            CHECK(a == a0 && b == b0 && c == c0 && e == e0);
        }
        // the sampler's CSRs: valid ones, and ones with an offset or an index overwritten
        const int64_t n_ctx = 1 + (int64_t)(rng() % 8), n_cand = 1 + (int64_t)(rng() % 7);
        const Csr pos = random_csr(rng, n_ctx, n_cand, 1);
        Csr forb = random_csr(rng, n_ctx, n_cand, 2);
        if (check_csr(n_ctx, n_cand, pos.ptr.data(), pos.idx.data(), nullptr)) return 1;
        Csr hurt = forb;
        if (rng() % 2)
            hurt.ptr[(size_t)(rng() % (uint64_t)(n_ctx + 1))] = (int64_t)(rng() % (hurt.idx.size() + 1));
        else if (!hurt.idx.empty())
            hurt.idx[(size_t)(rng() % hurt.idx.size())] = (int32_t)(rng() % (uint64_t)(n_cand + 2)) - 1;
        if (hurt.ptr.back() > (int64_t)hurt.idx.size()) hurt.ptr.back() = (int64_t)hurt.idx.size();
        if (check_csr(n_ctx, n_cand, hurt.ptr.data(), hurt.idx.empty() ? nullptr : hurt.idx.data(),
                      (const char*)-1))
            return 1;
        // positives against a random forbidden set, and against their union with it
        if (check_positives(n_cand, pos, forb, -1, -1)) return 1;
        Csr uni;
        uni.ptr.push_back(0);
        for (int64_t b = 0; b < n_ctx; ++b) {
            std::vector<char> on((size_t)n_cand, 0);
            for (int64_t e = pos.ptr[(size_t)b]; e < pos.ptr[(size_t)b + 1]; ++e) on[(size_t)pos.idx[(size_t)e]] = 1;
            for (int64_t e = forb.ptr[(size_t)b]; e < forb.ptr[(size_t)b + 1]; ++e) on[(size_t)forb.idx[(size_t)e]] = 1;
            for (int32_t j = 0; j < n_cand; ++j)
                if (on[(size_t)j]) uni.idx.push_back(j);
            uni.ptr.push_back((int64_t)uni.idx.size());
        }
        {
            int64_t row = -1;
            const int kind = check_positives_in_forbidden(n_ctx, n_cand, pos.ptr.data(),
                                                          pos.idx.data(), uni.ptr.data(),
                                                          uni.idx.data(), &row);
            CHECK(kind != kForbiddenLacksPositive);  // a superset never lacks a positive
            if (kind)
                CHECK(uni.ptr[(size_t)row + 1] - uni.ptr[(size_t)row] == n_cand &&
                      pos.ptr[(size_t)row + 1] > pos.ptr[(size_t)row]);
        }
        if (check_positives(n_cand, pos, uni, -1, -1)) return 1;
        // the column rule over a random CSC image and random sides
        const int32_t d = (int32_t)(rng() % 9);
        const int64_t rows = 1 + (int64_t)(rng() % 9);
        const Csr csc = random_csr(rng, d, rows, 1);
        std::vector<uint8_t> side((size_t)rows);
        for (uint8_t& s : side) s = (uint8_t)(rng() % 4);
        CHECK(first_shared_column(side, d, csc.ptr.data(), csc.idx.data()) ==
              old_shared_column(side, d, csc.ptr, csc.idx));
    }
    std::puts("ok");
    return 0;
}
