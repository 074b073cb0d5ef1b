// spfm_psgd_host.h -- the host-side rules of the minibatch unit (no HIP, no engine): step sizes,
// the tabulated epoch, the shares of a sharded epoch, and the argument checks of the pair fit and
// its sampler.  Kept apart so that a stand-alone program can run them under a host sanitizer
// (tools/check_psgd_host.cpp).  See DESIGN.md section 6.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace spfm {

// One minibatch as the kernels see it when a whole run of minibatches is replayed from a
// hipGraph (identical kernel arguments for every batch): the host tabulates the epoch
// (psgd.py:9-22 step sizes included) and two device counters walk through the table --
// the gradient kernel reads idx[0] and leaves idx[1] = that batch for the update kernel,
// which leaves idx[0] = batch + 1 when it is done.  Kernels on one stream run one after
// the other, so a counter is never written while a kernel that reads it is running.
struct PsgdBatch {
    long long pos;  // first position of the batch in the sample order
    int B;          // rows in the batch
    int pad;
    double cp, denp, strength, cw, denw;  // eta_P/B, 1+eta_P*beta, prox strength, eta_w/B, 1+eta_w*alpha
    // adaptive steps only (zero otherwise): what psgd_update_adaptive_kernel forms a column's
    // step from -- the base rates of this minibatch, the penalties as given, the accumulators'
    // offset G0.  They travel in the table so that a replayed graph never holds a stale one.
    double eta_P, eta_w, alpha, beta, gamma, g0;
};

// psgd.py:9-22
inline void psgd_eta(int lr, double eta0, double alpha, double beta, double power_t, int64_t it,
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

// Per-feature AdaGrad steps (spfm_psgd_set_adaptive): why a handle in
// adaptive mode cannot run an epoch, in the order the checks are made; nullptr: it can.
inline const char* psgd_adaptive_error(bool squared_norm, bool ranks, bool acc_fit) {
    if (squared_norm)
        return "adaptive steps cannot be combined with squaredl12 / squaredl21: their prox "
               "couples columns that now carry different steps";
    if (ranks) return "adaptive steps are not supported with several ranks";
    if (!acc_fit)
        return "the adaptive accumulators do not fit the parameters: call "
               "spfm_psgd_set_adaptive again";
    return nullptr;
}

// What an epoch entry passes down to the minibatches: filled once in the extern "C" entry.
struct PsgdStep {
    int degree;
    double alpha, beta, gamma, eta0;
    int lr;
    double power_t;
    int64_t batch_size;
    int fit_linear;
    int64_t* it;
    // the handle's adaptive mode (0: off), its G0, and psgd_adaptive_error() of its state
    int adaptive = 0;
    double g0 = 0.0;
    const char* adaptive_err = nullptr;

    // the step-argument checks in `what`'s words; empty: none failed
    std::string check(const char* what) const {
        const char* e = !it               ? "it is required"
                        : batch_size < 1   ? "batch_size must be >= 1"
                        : lr < 0 || lr > 3 ? "learning_rate is not supported."
                        : *it < 1          ? "it must be >= 1"
                        : adaptive         ? adaptive_err
                                           : nullptr;
        return e ? std::string(what) + ": " + e : std::string();
    }
    // the scalars of minibatch number `at` with B rows (pos is the caller's)
    PsgdBatch batch(int64_t at, int B) const {
        double eta_P, eta_w;
        psgd_eta(lr, eta0, alpha, beta, power_t, at, &eta_P, &eta_w);
        PsgdBatch e;
        e.pos = 0;
        e.B = B;
        e.pad = 0;
        e.cp = eta_P / (double)B;
        e.denp = 1.0 + eta_P * beta;
        e.strength = gamma * eta_P / (1 + eta_P * beta);
        e.cw = eta_w / (double)B;
        e.denw = 1 + eta_w * alpha;
        e.eta_P = adaptive ? eta_P : 0.0;
        e.eta_w = adaptive ? eta_w : 0.0;
        e.alpha = adaptive ? alpha : 0.0;
        e.beta = adaptive ? beta : 0.0;
        e.gamma = adaptive ? gamma : 0.0;
        e.g0 = adaptive ? g0 : 0.0;
        return e;
    }
};

// the minibatches of one epoch over n_items items, the first of them minibatch number it0
inline void tabulate_epoch(const PsgdStep& st, int64_t n_items, int64_t it0,
                           std::vector<PsgdBatch>& out) {
    const int64_t nbat = (n_items + st.batch_size - 1) / st.batch_size;
    out.resize((size_t)nbat);
    for (int64_t bi = 0; bi < nbat; ++bi) {
        const int64_t pos = bi * st.batch_size;
        out[(size_t)bi] = st.batch(it0 + bi, (int)std::min<int64_t>(st.batch_size, n_items - pos));
        out[(size_t)bi].pos = pos;
    }
}

// Several ranks: per minibatch of the GLOBAL order the samples of the rank that holds rows
// [row_lo, row_lo + n) -- first position in its local list `local`, count -- and the global batch
// size.  False: the order does not hold each of the rank's rows once.
inline bool shard_batches(const int32_t* order, int64_t n_global, int64_t row_lo, int64_t n,
                          int64_t batch_size, std::vector<int64_t>& lpos, std::vector<int32_t>& lB,
                          std::vector<int32_t>& gB, std::vector<int32_t>& local) {
    const int64_t nbat = (n_global + batch_size - 1) / batch_size;
    lpos.assign((size_t)nbat, 0);
    lB.assign((size_t)nbat, 0);
    gB.assign((size_t)nbat, 0);
    local.clear();
    local.reserve((size_t)n);
    for (int64_t bi = 0; bi < nbat; ++bi) {
        const int64_t pos = bi * batch_size;
        const int64_t B = std::min<int64_t>(batch_size, n_global - pos);
        lpos[(size_t)bi] = (int64_t)local.size();
        for (int64_t q = pos; q < pos + B; ++q) {
            const int64_t i = (int64_t)order[q] - row_lo;
            if (i >= 0 && i < n) local.push_back((int32_t)i);
        }
        lB[(size_t)bi] = (int32_t)((int64_t)local.size() - lpos[(size_t)bi]);
        gB[(size_t)bi] = (int32_t)B;
    }
    return (int64_t)local.size() == n;
}

// list[0, m) holds each of 0..m-1 once
inline bool is_permutation(const int32_t* list, int64_t m) {
    std::vector<char> seen((size_t)m, 0);
    for (int64_t q = 0; q < m; ++q) {
        const int32_t i = list[q];
        if (i < 0 || i >= m || seen[(size_t)i]) return false;
        seen[(size_t)i] = 1;
    }
    return true;
}

// one CSR over n_cand columns: in range, strictly ascending within a row
inline const char* sampler_csr_error(int64_t rows, int64_t n_cand, const int64_t* ptr,
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

// Two valid CSRs: every row with a positive must hold its positives in its forbidden list and
// leave a candidate free.  Returns 0, or the kind of the first violation with its row in *row:
enum { kForbiddenLacksPositive = 1, kForbidsEveryCandidate = 2 };
inline int check_positives_in_forbidden(int64_t n_ctx, int64_t n_cand, const int64_t* pos_ptr,
                                        const int32_t* pos_idx, const int64_t* forb_ptr,
                                        const int32_t* forb_idx, int64_t* row) {
    for (int64_t b = 0; b < n_ctx; ++b) {
        if (pos_ptr[b + 1] == pos_ptr[b]) continue;
        *row = b;
        int64_t f = forb_ptr[b];
        const int64_t f1 = forb_ptr[b + 1];
        for (int64_t e = pos_ptr[b]; e < pos_ptr[b + 1]; ++e) {  // both sorted: one merge
            while (f < f1 && forb_idx[f] < pos_idx[e]) ++f;
            if (f == f1 || forb_idx[f] != pos_idx[e]) return kForbiddenLacksPositive;
        }
        if (f1 - forb_ptr[b] >= n_cand) return kForbidsEveryCandidate;
    }
    return 0;
}

// The disjoint-column rule of the pair fit.  side[row]: 1 = context side, 2 = candidate side, 3 =
// both, 0 = unused.  The first column (of the CSC image cptr / cidx) stored on both sides; -1: none.
inline int32_t first_shared_column(const std::vector<uint8_t>& side, int32_t d, const int64_t* cptr,
                                   const int32_t* cidx) {
    for (int32_t j = 0; j < d; ++j) {
        unsigned both = 0;
        for (int64_t e = cptr[j]; e < cptr[j + 1]; ++e) both |= side[(size_t)cidx[e]];
        if (both == 3) return j;
    }
    return -1;
}

}  // namespace spfm
