// spfm_engine_interactions.hip -- spfm_interaction_stats / _topk / _list / _values / _block and
// spfm_interaction3_stats / _topk / _list / _values (include/spfm.h): which feature pairs and
// triples the model kept, from the live device parameters.
// W = P_o^T diag(lams) P_o is formed tile by tile in registers and consumed there, and so is
// T[a, j, l] = sum_s lams_s p_sa p_sj p_sl, pivot by pivot on the same tiles; nothing of size
// d_a^2 or d_a^3 is allocated.  Stats, select and list are written once, against an IntPass that
// says what a pass over pairs or over triples is.  All entries are read-only views like the
// objective unit: scratch buffers of their own (one set for both orders), no change to the
// P / Pt validity flags, to y_pred, the regularizer state or the schedule.  See DESIGN.md
// sections 14 and 14a.
#include "spfm_engine.hip.h"
#include "spfm_interactions3.hip.h"
#include "spfm_interactions_host.h"

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

static_assert(kInt3KeyBits == kInt3IdBits, "host and device agree on the key");

// the live image of block `order_idx` (obj_block_kernel's view), behind the entries' checks
int spfm_engine::interaction_view(const char* what, int order_idx, BlockView* v) {
    if (!have_params) FAIL(SPFM_ERR_INVALID, std::string(what) + ": no parameters set");
    if (order_idx < 0 || order_idx >= n_orders)
        FAIL(SPFM_ERR_INVALID, std::string(what) + ": bad order index");
    *v = live_block(order_idx);
    return SPFM_OK;
}

// compaction: int_ids, the packed images int_A / int_B, int_da / int_kp / int_T
int spfm_engine::interaction_prepare(const char* what, int order_idx) {
    BlockView v;
    int rc = interaction_view(what, order_idx, &v);
    if (rc) return rc;
    const double* base = v.base;
    const int64_t ss = v.ss, sj = v.sj;
    const int dlim = (int_dlim > 0 && int_dlim < d) ? int_dlim : d;
    const unsigned nb = cdiv(d, kBlock);
    HIPC(int_flag.alloc(sizeof(int32_t) * (size_t)d));
    HIPC(int_pos.alloc(sizeof(int32_t) * (size_t)d));
    // (padded to whole tiles: the tile kernel indexes it with padded rows only behind a test
    // that a zero row never passes)
    const size_t ids_n = (size_t)cdiv(d, kIntTile) * kIntTile;
    HIPC(int_ids.alloc(sizeof(int32_t) * ids_n));
    HIPC(int_tot.alloc(sizeof(int32_t) * 4));
    HIPC(hipMemsetAsync(int_ids.p, 0, sizeof(int32_t) * ids_n, stream));
    hipLaunchKernelGGL(int_flag_kernel, dim3(nb), dim3(kBlock), 0, stream, base, ss, sj, k, d, dlim,
                       int_flag.as<int32_t>());
    size_t temp_bytes = 0;
    HIPC(rocprim::exclusive_scan(nullptr, temp_bytes, int_flag.as<int32_t>(),
                                 int_pos.as<int32_t>(), (int32_t)0, (size_t)d,
                                 rocprim::plus<int32_t>(), stream));
    HIPC(int_tmp.alloc(temp_bytes));
    HIPC(rocprim::exclusive_scan(int_tmp.p, temp_bytes, int_flag.as<int32_t>(),
                                 int_pos.as<int32_t>(), (int32_t)0, (size_t)d,
                                 rocprim::plus<int32_t>(), stream));
    hipLaunchKernelGGL(int_compact_kernel, dim3(nb), dim3(kBlock), 0, stream,
                       int_flag.as<int32_t>(), int_pos.as<int32_t>(), d, int_ids.as<int32_t>(),
                       int_tot.as<int32_t>());
    HIPC(hipGetLastError());
    int32_t da = 0;
    SPFM_TRY(download(&da, int_tot.p, 1));
    rc = sync();
    if (rc) return rc;
    if (da < 0 || da > d) FAIL(SPFM_ERR_RUNTIME, std::string(what) + ": compaction failed");
    int_da = da;
    int_kp = (k + 3) / 4 * 4;
    int_T = (int)cdiv(da, kIntTile);
    if (da < 2) return SPFM_OK;  // no pair
    const int64_t total = (int64_t)int_T * kIntTile * int_kp;
    HIPC(int_A.alloc(sizeof(double) * (size_t)total));
    HIPC(int_B.alloc(sizeof(double) * (size_t)total));
    hipLaunchKernelGGL(int_pack_kernel, dim3(cdiv(total, kBlock)), dim3(kBlock), 0, stream, base,
                       ss, sj, k, int_kp, da, total, int_ids.as<int32_t>(), lams.as<double>(),
                       int_A.as<double>(), int_B.as<double>());
    HIPC(hipGetLastError());
    return SPFM_OK;
}

IntArgs spfm_engine::interaction_args() {
    IntArgs a;
    memset(&a, 0, sizeof a);
    a.A = int_A.as<double>();
    a.B = int_B.as<double>();
    a.ids = int_ids.as<int32_t>();
    a.kp = int_kp;
    a.T = int_T;
    a.prefix_shift = 64;
    return a;
}

// the pair unit's compaction, then the work guard: before any product pass
int spfm_engine::interaction3_prepare(const char* what, int order_idx) {
    int rc = interaction_prepare(what, order_idx);
    if (rc) return rc;
    if (int_da > SPFM_INTERACTION3_MAX_ACTIVE) {
        char buf[256];
        snprintf(buf, sizeof buf,
                 "%s: d_a = %d active features in view, more than SPFM_INTERACTION3_MAX_ACTIVE = "
                 "%d (a pass is d_a^3 k / 3 flops); narrow the view with the option "
                 "\"interaction_features\"",
                 what, int_da, (int)SPFM_INTERACTION3_MAX_ACTIVE);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    return SPFM_OK;
}

void spfm_engine::interaction_release() {
    for (DevBuf* b : {&int_flag, &int_pos, &int_ids, &int_tot, &int_tmp, &int_A, &int_B, &int_rec,
                      &int_rec2, &int_hist, &int_cnt, &int_keys, &int_vals, &int_keys2,
                      &int_vals2, &int_io, &int_out, &int_pq, &int_pqr, &int_prec, &int_pdeg,
                      &int_pon})
        b->release();
    int_psel.release();
}

// What a pass is; the driver below reads these and interprets none of them.
struct IntPass {
    const char* prefix;  // of the entry names in messages
    const char* noun;    // what is counted, in messages
    int min_da;          // least d_a with any work
    int64_t (*units)(int T);  // workgroups of a whole pass over T tiles per side
    int64_t window;      // units whose records exist at a time (whole runs of kIntRun)
    int64_t budget;      // units per launch without the option "interaction_tile_budget"; today a
                         // window in both passes, but a launch need not be one
    int key_bits;        // bits of an emitted key that the list sorts
    // the units [a.tile0, a.tile0 + n) in mode INT_STATS / INT_HIST / INT_EMIT
    void (*launch[3])(const IntArgs& a, int da, unsigned n, hipStream_t stream);
    // emitted keys -> the caller's id arrays
    int (spfm_engine::*unpack)(const uint64_t* keys, size_t n, int32_t* const* ids);
};

template <int MODE>
static void int_launch(const IntArgs& a, int, unsigned n, hipStream_t stream) {
    hipLaunchKernelGGL((int_tile_kernel<MODE>), dim3(n), dim3(kBlock), 0, stream, a);
}

template <int MODE>
static void int3_launch(const IntArgs& a, int da, unsigned n, hipStream_t stream) {
    hipLaunchKernelGGL((int3_tile_kernel<MODE>), dim3(n), dim3(kBlock), 0, stream,
                       Int3Args{a, da});
}

// pairs: the upper-triangular tiles; keys hold feature ids
static const IntPass kPairPass = {
    "interaction", "pairs", 2, [](int T) { return (int64_t)T * (T + 1) / 2; },
    kIntWindow, kIntWindow, 64,
    {int_launch<INT_STATS>, int_launch<INT_HIST>, int_launch<INT_EMIT>},
    &spfm_engine::interaction_unpack};
// triples: (pair tile, pivot block) units; keys hold compacted ids
static const IntPass kTriplePass = {
    "interaction3", "triples", 3, [](int T) { return (int64_t)int3_units_before(T, T); },
    kInt3Window, kInt3Window, 3 * kInt3IdBits,
    {int3_launch<INT_STATS>, int3_launch<INT_HIST>, int3_launch<INT_EMIT>},
    &spfm_engine::interaction3_unpack};

int spfm_engine::interaction_unpack(const uint64_t* keys, size_t n, int32_t* const* ids) {
    for (size_t q = 0; q < n; ++q) int_split_key(keys[q], ids[0] + q, ids[1] + q);
    return SPFM_OK;
}

// keys of compacted ids -> feature ids (int_ids of the last compaction)
int spfm_engine::interaction3_unpack(const uint64_t* keys, size_t n, int32_t* const* out) {
    std::vector<int32_t> ids((size_t)int_da);
    SPFM_TRY(download(ids.data(), int_ids.p, ids.size()));
    SPFM_TRY(sync());
    for (size_t q = 0; q < n; ++q)
        if (!int3_unpack_key(keys[q], ids.data(), int_da, out[0] + q, out[1] + q, out[2] + q))
            FAIL(SPFM_ERR_RUNTIME, "interaction3: emitted id out of range");
    return SPFM_OK;
}

// the units [u0, u1) in `mode`, at most `interaction_tile_budget` of them per launch
int spfm_engine::interaction_run(const IntPass& ps, int mode, IntArgs a, int64_t u0, int64_t u1) {
    const int64_t per = int_tile_budget > 0 ? int_tile_budget : ps.budget;
    for (; u0 < u1; u0 += per) {
        a.tile0 = u0;
        ps.launch[mode](a, int_da, (unsigned)std::min<int64_t>(per, u1 - u0), stream);
        ++int_launches;
    }
    HIPC(hipGetLastError());
    return SPFM_OK;
}

// a whole pass
int spfm_engine::interaction_run(const IntPass& ps, int mode, IntArgs a) {
    int_launches = 0;
    return interaction_run(ps, mode, a, 0, ps.units(int_T));
}

int spfm_engine::interaction_pass_stats(const IntPass& ps, double tol, int64_t* counts2,
                                        double* sums3) {
    counts2[0] = 0;
    counts2[1] = int_da;
    sums3[0] = sums3[1] = sums3[2] = 0.0;
    if (int_da < ps.min_da) return SPFM_OK;
    // Unit records live for one window (a multiple of the run length) and are combined into one
    // record per run of kIntRun units right away; the runs are then combined level by level.  The
    // tree depends on the unit count alone, not on the launch partition.
    const int64_t nunit = ps.units(int_T);
    const int64_t n1 = (nunit + kIntRun - 1) / kIntRun;
    HIPC(int_rec.alloc(sizeof(IntRec) * (size_t)std::min<int64_t>(nunit, ps.window)));
    HIPC(int_rec2.alloc(sizeof(IntRec) * (size_t)(n1 + (n1 + kIntRun - 1) / kIntRun + 2)));
    IntRec* lvl[2] = {int_rec2.as<IntRec>(), int_rec2.as<IntRec>() + n1};
    IntArgs a = interaction_args();
    a.tol = tol;
    int_launches = 0;
    for (int64_t w0 = 0; w0 < nunit; w0 += ps.window) {
        const int64_t w1 = std::min<int64_t>(nunit, w0 + ps.window);
        a.rec = int_rec.as<IntRec>();
        a.rec_base = w0;
        SPFM_TRY(interaction_run(ps, INT_STATS, a, w0, w1));
        hipLaunchKernelGGL(int_reduce_kernel, dim3((unsigned)((w1 - w0 + kIntRun - 1) / kIntRun)),
                           dim3(kBlock), 0, stream, int_rec.as<IntRec>(), (long long)(w1 - w0),
                           lvl[0] + w0 / kIntRun);
    }
    const IntRec* in = lvl[0];
    int64_t nin = n1;
    int which = 1;
    while (nin > 1) {
        const int64_t nout = (nin + kIntRun - 1) / kIntRun;
        hipLaunchKernelGGL(int_reduce_kernel, dim3((unsigned)nout), dim3(kBlock), 0, stream, in,
                           (long long)nin, lvl[which]);
        in = lvl[which];
        nin = nout;
        which ^= 1;
    }
    HIPC(hipGetLastError());
    IntRec out;
    SPFM_TRY(download(&out, in, 1));
    SPFM_TRY(sync());
    counts2[0] = out.cnt;
    sums3[0] = out.sumsq;
    sums3[1] = out.sumabs;
    sums3[2] = out.maxabs;
    return SPFM_OK;
}

// INT_EMIT into int_keys / int_vals (capacity `cap`); *n_found = the values that qualified
int spfm_engine::interaction_emit(const IntPass& ps, double tol, unsigned long long thr_key,
                                  int64_t cap, int64_t* n_found) {
    HIPC(int_keys.alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(cap, 1)));
    HIPC(int_vals.alloc(sizeof(double) * (size_t)std::max<int64_t>(cap, 1)));
    HIPC(int_cnt.alloc(sizeof(uint64_t)));
    HIPC(hipMemsetAsync(int_cnt.p, 0, sizeof(uint64_t), stream));
    IntArgs a = interaction_args();
    a.tol = tol;
    a.thr_key = thr_key;
    a.cap = (unsigned long long)cap;
    a.counter = int_cnt.as<unsigned long long>();
    a.keys = int_keys.as<unsigned long long>();
    a.vals = int_vals.as<double>();
    SPFM_TRY(interaction_run(ps, INT_EMIT, a));
    uint64_t found = 0;
    SPFM_TRY(download(&found, int_cnt.p, 1));
    SPFM_TRY(sync());
    *n_found = (int64_t)found;
    return SPFM_OK;
}

int spfm_engine::interaction_pass_topk(const IntPass& ps, int64_t K, int32_t* const* ids,
                                       double* vals, int64_t* n_out) {
    if (K == 0 || int_da < ps.min_da) return SPFM_OK;
    // Radix select on the f64 pattern of the magnitude (monotone once the sign is dropped): per
    // level a histogram of the next bits among the values whose higher bits equal the prefix found
    // so far; the bin whose tail first holds K values extends the prefix.  Counts are exact, so
    // the size of the candidate set is known before it is emitted.
    static const int shifts[6] = {52, 40, 28, 16, 4, 0};
    static const int bits[6] = {12, 12, 12, 12, 12, 4};
    const int64_t soft = std::max<int64_t>(2 * K, 65536);     // refine while the tail is larger
    const int64_t hard = std::max<int64_t>(2 * K, 1 << 20);   // candidate buffer bound
    HIPC(int_hist.alloc(sizeof(uint64_t) * kIntHistBins));
    std::vector<uint64_t> hh(kIntHistBins);
    unsigned long long prefix = 0, thr_key = 0;
    int prefix_shift = 64;
    int64_t above = 0, tail = 0;
    for (int L = 0; L < 6; ++L) {
        HIPC(hipMemsetAsync(int_hist.p, 0, sizeof(uint64_t) * kIntHistBins, stream));
        IntArgs a = interaction_args();
        a.hist = int_hist.as<unsigned long long>();
        a.prefix = prefix;
        a.prefix_shift = prefix_shift;
        a.bin_shift = shifts[L];
        a.bin_mask = (1u << bits[L]) - 1u;
        SPFM_TRY(interaction_run(ps, INT_HIST, a));
        SPFM_TRY(download(hh.data(), int_hist.p, hh.size()));
        SPFM_TRY(sync());
        int64_t above_next = 0;
        const int b = int_select_bin(hh.data(), 1 << bits[L], above, K, &tail, &above_next);
        if (b < 0) {  // (first level only) fewer than K non-zero values: all of them
            thr_key = 0;
            break;
        }
        prefix = (prefix << bits[L]) | (unsigned long long)b;
        thr_key = prefix << shifts[L];
        above = above_next;
        prefix_shift = shifts[L];
        if (tail <= soft) break;
    }
    if (tail == 0) return SPFM_OK;
    if (tail > hard) {
        char buf[160];
        snprintf(buf, sizeof buf,
                 "%s_topk: %lld %s tie with the K-th magnitude (candidate bound %lld)", ps.prefix,
                 (long long)tail, ps.noun, (long long)hard);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    int64_t found = 0;
    SPFM_TRY(interaction_emit(ps, 0.0, thr_key, tail, &found));
    if (found != tail)
        FAIL(SPFM_ERR_RUNTIME, std::string(ps.prefix) + "_topk: candidate count mismatch");
    std::vector<uint64_t> hk((size_t)tail);
    std::vector<double> hv((size_t)tail);
    SPFM_TRY(download(hk.data(), int_keys.p, hk.size()));
    SPFM_TRY(download(hv.data(), int_vals.p, hv.size()));
    SPFM_TRY(sync());
    // magnitude descending, then the ids ascending (either key orders its ids; compaction is
    // monotone)
    std::vector<int64_t> idx;
    const int64_t nk = int_order_candidates(hk, hv, K, idx);
    std::vector<uint64_t> top((size_t)nk);
    for (int64_t q = 0; q < nk; ++q) {
        top[(size_t)q] = hk[(size_t)idx[(size_t)q]];
        vals[q] = hv[(size_t)idx[(size_t)q]];
    }
    SPFM_TRY((this->*ps.unpack)(top.data(), top.size(), ids));
    *n_out = nk;
    return SPFM_OK;
}

int spfm_engine::interaction_pass_list(const IntPass& ps, double tol, int64_t capacity,
                                       int32_t* const* ids, double* vals, int64_t* n_out) {
    if (int_da < ps.min_da) return SPFM_OK;
    int64_t found = 0;
    SPFM_TRY(interaction_emit(ps, tol, 0ull, capacity, &found));
    *n_out = found;
    if (found > capacity) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s_list: %lld %s above tol, capacity %lld", ps.prefix,
                 (long long)found, ps.noun, (long long)capacity);
        FAIL(SPFM_ERR_INVALID, buf);
    }
    if (found == 0) return SPFM_OK;
    // sorted by the ids = by key: the emission order does not matter
    const size_t nf = (size_t)found;
    HIPC(int_keys2.alloc(sizeof(uint64_t) * nf));
    HIPC(int_vals2.alloc(sizeof(double) * nf));
    size_t temp_bytes = 0;
    HIPC(rocprim::radix_sort_pairs(nullptr, temp_bytes, int_keys.as<uint64_t>(),
                                   int_keys2.as<uint64_t>(), int_vals.as<double>(),
                                   int_vals2.as<double>(), nf, 0, ps.key_bits, stream));
    HIPC(int_tmp.alloc(temp_bytes));
    HIPC(rocprim::radix_sort_pairs(int_tmp.p, temp_bytes, int_keys.as<uint64_t>(),
                                   int_keys2.as<uint64_t>(), int_vals.as<double>(),
                                   int_vals2.as<double>(), nf, 0, ps.key_bits, stream));
    std::vector<uint64_t> hk(nf);
    std::vector<double> hv(nf);  // the caller's arrays are written only once nothing can fail
    SPFM_TRY(download(hk.data(), int_keys2.p, nf));
    SPFM_TRY(download(hv.data(), int_vals2.p, nf));
    SPFM_TRY(sync());
    SPFM_TRY((this->*ps.unpack)(hk.data(), nf, ids));
    std::copy(hv.begin(), hv.end(), vals);
    return SPFM_OK;
}

// ---- the entries: argument checks, compaction, one driver call
int spfm_engine::interaction_stats(int order_idx, double tol, int64_t* counts2, double* sums3) {
    if (!counts2 || !sums3) FAIL(SPFM_ERR_INVALID, "interaction_stats: NULL output");
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction_stats: tol must be >= 0");
    SPFM_TRY(interaction_prepare("interaction_stats", order_idx));
    return interaction_pass_stats(kPairPass, tol, counts2, sums3);
}

int spfm_engine::interaction3_stats(int order_idx, double tol, int64_t* counts2, double* sums3) {
    if (!counts2 || !sums3) FAIL(SPFM_ERR_INVALID, "interaction3_stats: NULL output");
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction3_stats: tol must be >= 0");
    SPFM_TRY(interaction3_prepare("interaction3_stats", order_idx));
    return interaction_pass_stats(kTriplePass, tol, counts2, sums3);
}

int spfm_engine::interaction_topk(int order_idx, int64_t K, int32_t* rows, int32_t* cols,
                                  double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction_topk: n_out is NULL");
    *n_out = 0;
    if (K < 0) FAIL(SPFM_ERR_INVALID, "interaction_topk: K must be >= 0");
    if (K > ((int64_t)1 << 28)) FAIL(SPFM_ERR_UNSUPPORTED, "interaction_topk: K must be <= 2^28");
    if (K > 0 && (!rows || !cols || !vals)) FAIL(SPFM_ERR_INVALID, "interaction_topk: NULL output");
    SPFM_TRY(interaction_prepare("interaction_topk", order_idx));
    int32_t* const ids[2] = {rows, cols};
    return interaction_pass_topk(kPairPass, K, ids, vals, n_out);
}

int spfm_engine::interaction3_topk(int order_idx, int64_t K, int32_t* i, int32_t* j, int32_t* l,
                                   double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction3_topk: n_out is NULL");
    *n_out = 0;
    if (K < 0) FAIL(SPFM_ERR_INVALID, "interaction3_topk: K must be >= 0");
    if (K > ((int64_t)1 << 28)) FAIL(SPFM_ERR_UNSUPPORTED, "interaction3_topk: K must be <= 2^28");
    if (K > 0 && (!i || !j || !l || !vals)) FAIL(SPFM_ERR_INVALID, "interaction3_topk: NULL output");
    SPFM_TRY(interaction3_prepare("interaction3_topk", order_idx));
    int32_t* const ids[3] = {i, j, l};
    return interaction_pass_topk(kTriplePass, K, ids, vals, n_out);
}

int spfm_engine::interaction_list(int order_idx, double tol, int64_t capacity, int32_t* rows,
                                  int32_t* cols, double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction_list: n_out is NULL");
    *n_out = 0;
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction_list: tol must be >= 0");
    if (capacity < 0) FAIL(SPFM_ERR_INVALID, "interaction_list: capacity must be >= 0");
    if (capacity > 0 && (!rows || !cols || !vals))
        FAIL(SPFM_ERR_INVALID, "interaction_list: NULL output");
    SPFM_TRY(interaction_prepare("interaction_list", order_idx));
    int32_t* const ids[2] = {rows, cols};
    return interaction_pass_list(kPairPass, tol, capacity, ids, vals, n_out);
}

int spfm_engine::interaction3_list(int order_idx, double tol, int64_t capacity, int32_t* i,
                                   int32_t* j, int32_t* l, double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction3_list: n_out is NULL");
    *n_out = 0;
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction3_list: tol must be >= 0");
    if (capacity < 0) FAIL(SPFM_ERR_INVALID, "interaction3_list: capacity must be >= 0");
    if (capacity > 0 && (!i || !j || !l || !vals))
        FAIL(SPFM_ERR_INVALID, "interaction3_list: NULL output");
    SPFM_TRY(interaction3_prepare("interaction3_list", order_idx));
    int32_t* const ids[3] = {i, j, l};
    return interaction_pass_list(kTriplePass, tol, capacity, ids, vals, n_out);
}

int spfm_engine::interaction_values(int order_idx, int64_t L, const int32_t* rows,
                                    const int32_t* cols, double* vals) {
    if (L < 0) FAIL(SPFM_ERR_INVALID, "interaction_values: L must be >= 0");
    if (L > 0 && (!rows || !cols || !vals)) FAIL(SPFM_ERR_INVALID, "interaction_values: NULL array");
    BlockView v;
    SPFM_TRY(interaction_view("interaction_values", order_idx, &v));
    for (int64_t q = 0; q < L; ++q)
        if (rows[q] < 0 || rows[q] >= d || cols[q] < 0 || cols[q] >= d)
            FAIL(SPFM_ERR_INVALID, "interaction_values: feature id out of range");
    if (L == 0) return SPFM_OK;
    HIPC(int_io.alloc(sizeof(int32_t) * 2 * (size_t)L));
    HIPC(int_out.alloc(sizeof(double) * (size_t)L));
    int32_t* dr = int_io.as<int32_t>();
    int32_t* dc = dr + L;
    SPFM_TRY(upload_to(dr, rows, (size_t)L));
    SPFM_TRY(upload_to(dc, cols, (size_t)L));
    hipLaunchKernelGGL(int_values_kernel, dim3(cdiv(L, kBlock)), dim3(kBlock), 0, stream, v.base,
                       v.ss, v.sj, k, lams.as<double>(), (long long)L, dr, dc, int_out.as<double>());
    HIPC(hipGetLastError());
    SPFM_TRY(download(vals, int_out.p, (size_t)L));
    return sync();
}

int spfm_engine::interaction_block(int order_idx, int64_t nJ, const int32_t* J, int64_t nJ2,
                                   const int32_t* J2, double* out) {
    if (nJ < 0 || nJ2 < 0) FAIL(SPFM_ERR_INVALID, "interaction_block: negative size");
    if ((nJ > 0 && !J) || (nJ2 > 0 && !J2)) FAIL(SPFM_ERR_INVALID, "interaction_block: NULL array");
    BlockView v;
    SPFM_TRY(interaction_view("interaction_block", order_idx, &v));
    for (int64_t q = 0; q < nJ; ++q)
        if (J[q] < 0 || J[q] >= d)
            FAIL(SPFM_ERR_INVALID, "interaction_block: feature id out of range");
    for (int64_t q = 0; q < nJ2; ++q)
        if (J2[q] < 0 || J2[q] >= d)
            FAIL(SPFM_ERR_INVALID, "interaction_block: feature id out of range");
    if (nJ == 0 || nJ2 == 0) return SPFM_OK;
    if ((double)nJ * (double)nJ2 * 8.0 > (double)SPFM_INTERACTION_BLOCK_MAX_BYTES) {
        char buf[160];
        snprintf(buf, sizeof buf,
                 "interaction_block: %lld x %lld doubles exceed the budget of %lld bytes",
                 (long long)nJ, (long long)nJ2, (long long)SPFM_INTERACTION_BLOCK_MAX_BYTES);
        FAIL(SPFM_ERR_INVALID, buf);
    }
    if (!out) FAIL(SPFM_ERR_INVALID, "interaction_block: out is NULL");
    const int64_t tot = nJ * nJ2;
    HIPC(int_io.alloc(sizeof(int32_t) * (size_t)(nJ + nJ2)));
    HIPC(int_out.alloc(sizeof(double) * (size_t)tot));
    int32_t* dj = int_io.as<int32_t>();
    int32_t* dj2 = dj + nJ;
    SPFM_TRY(upload_to(dj, J, (size_t)nJ));
    SPFM_TRY(upload_to(dj2, J2, (size_t)nJ2));
    hipLaunchKernelGGL(int_block_kernel, dim3(cdiv(tot, kBlock)), dim3(kBlock), 0, stream, v.base,
                       v.ss, v.sj, k, lams.as<double>(), (long long)nJ, dj, (long long)nJ2, dj2,
                       int_out.as<double>());
    HIPC(hipGetLastError());
    SPFM_TRY(download(out, int_out.p, (size_t)tot));
    return sync();
}

int spfm_engine::interaction3_values(int order_idx, int64_t L, const int32_t* i, const int32_t* j,
                                     const int32_t* l, double* vals) {
    if (L < 0) FAIL(SPFM_ERR_INVALID, "interaction3_values: L must be >= 0");
    if (L > 0 && (!i || !j || !l || !vals)) FAIL(SPFM_ERR_INVALID, "interaction3_values: NULL array");
    BlockView v;
    SPFM_TRY(interaction_view("interaction3_values", order_idx, &v));
    for (int64_t q = 0; q < L; ++q)
        if (i[q] < 0 || i[q] >= d || j[q] < 0 || j[q] >= d || l[q] < 0 || l[q] >= d)
            FAIL(SPFM_ERR_INVALID, "interaction3_values: feature id out of range");
    if (L == 0) return SPFM_OK;
    HIPC(int_io.alloc(sizeof(int32_t) * 3 * (size_t)L));
    HIPC(int_out.alloc(sizeof(double) * (size_t)L));
    int32_t* di = int_io.as<int32_t>();
    int32_t* dj = di + L;
    int32_t* dl = dj + L;
    SPFM_TRY(upload_to(di, i, (size_t)L));
    SPFM_TRY(upload_to(dj, j, (size_t)L));
    SPFM_TRY(upload_to(dl, l, (size_t)L));
    hipLaunchKernelGGL(int3_values_kernel, dim3(cdiv(L, kBlock)), dim3(kBlock), 0, stream, v.base,
                       v.ss, v.sj, k, lams.as<double>(), (long long)L, di, dj, dl,
                       int_out.as<double>());
    HIPC(hipGetLastError());
    SPFM_TRY(download(vals, int_out.p, (size_t)L));
    return sync();
}

extern "C" {

int spfm_interaction_stats(spfm_handle h, int order_idx, double tol, int64_t* counts2,
                           double* sums3) {
    SPFM_GUARD(h);
    return h->interaction_stats(order_idx, tol, counts2, sums3);
}

int spfm_interaction_topk(spfm_handle h, int order_idx, int64_t K, int32_t* rows, int32_t* cols,
                          double* vals, int64_t* n_out) {
    SPFM_GUARD(h);
    return h->interaction_topk(order_idx, K, rows, cols, vals, n_out);
}

int spfm_interaction_list(spfm_handle h, int order_idx, double tol, int64_t capacity,
                          int32_t* rows, int32_t* cols, double* vals, int64_t* n_out) {
    SPFM_GUARD(h);
    return h->interaction_list(order_idx, tol, capacity, rows, cols, vals, n_out);
}

int spfm_interaction_values(spfm_handle h, int order_idx, int64_t L, const int32_t* rows,
                            const int32_t* cols, double* vals) {
    SPFM_GUARD(h);
    return h->interaction_values(order_idx, L, rows, cols, vals);
}

int spfm_interaction_block(spfm_handle h, int order_idx, int64_t nJ, const int32_t* J,
                           int64_t nJ2, const int32_t* J2, double* out) {
    SPFM_GUARD(h);
    return h->interaction_block(order_idx, nJ, J, nJ2, J2, out);
}

int spfm_interaction3_stats(spfm_handle h, int order_idx, double tol, int64_t* counts2,
                            double* sums3) {
    SPFM_GUARD(h);
    return h->interaction3_stats(order_idx, tol, counts2, sums3);
}

int spfm_interaction3_topk(spfm_handle h, int order_idx, int64_t K, int32_t* i, int32_t* j,
                           int32_t* l, double* vals, int64_t* n_out) {
    SPFM_GUARD(h);
    return h->interaction3_topk(order_idx, K, i, j, l, vals, n_out);
}

int spfm_interaction3_list(spfm_handle h, int order_idx, double tol, int64_t capacity, int32_t* i,
                           int32_t* j, int32_t* l, double* vals, int64_t* n_out) {
    SPFM_GUARD(h);
    return h->interaction3_list(order_idx, tol, capacity, i, j, l, vals, n_out);
}

int spfm_interaction3_values(spfm_handle h, int order_idx, int64_t L, const int32_t* i,
                             const int32_t* j, const int32_t* l, double* vals) {
    SPFM_GUARD(h);
    return h->interaction3_values(order_idx, L, i, j, l, vals);
}

}  // extern "C"
