// spfm_engine_interactions.hip -- spfm_interaction_stats / _topk / _list / _values / _block
// (include/spfm.h): which feature pairs the model kept, from the live device parameters.
// W = P_o^T diag(lams) P_o is formed tile by tile in registers and consumed there; nothing of
// size d_a^2 is allocated.  All entries are read-only views like the objective unit: scratch
// buffers of their own, no change to the P / Pt validity flags, to y_pred, the regularizer state
// or the schedule.  See DESIGN.md section 14.
#include "spfm_engine.hip.h"
#include "spfm_interactions.hip.h"

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

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

// the upper-triangular tiles [t0, t1), at most `interaction_tile_budget` of them per launch
template <int MODE>
int spfm_engine::interaction_tiles(IntArgs a, int64_t t0, int64_t t1) {
    const int64_t per = int_tile_budget > 0 ? int_tile_budget : kIntWindow;
    for (; t0 < t1; t0 += per) {
        a.tile0 = t0;
        const int64_t nt = std::min<int64_t>(per, t1 - t0);
        hipLaunchKernelGGL((int_tile_kernel<MODE>), dim3((unsigned)nt), dim3(kBlock), 0, stream, a);
        ++int_launches;
    }
    HIPC(hipGetLastError());
    return SPFM_OK;
}

template <int MODE>
int spfm_engine::interaction_tiles(IntArgs a) {
    int_launches = 0;
    return interaction_tiles<MODE>(a, 0, (int64_t)int_T * (int_T + 1) / 2);
}

void spfm_engine::interaction_release() {
    for (DevBuf* b : {&int_flag, &int_pos, &int_ids, &int_tot, &int_tmp, &int_A, &int_B, &int_rec,
                      &int_rec2, &int_hist, &int_cnt, &int_keys, &int_vals, &int_keys2,
                      &int_vals2, &int_io, &int_out})
        b->release();
}

int spfm_engine::interaction_stats(int order_idx, double tol, int64_t* counts2, double* sums3) {
    if (!counts2 || !sums3) FAIL(SPFM_ERR_INVALID, "interaction_stats: NULL output");
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction_stats: tol must be >= 0");
    int rc = interaction_prepare("interaction_stats", order_idx);
    if (rc) return rc;
    counts2[0] = 0;
    counts2[1] = int_da;
    sums3[0] = sums3[1] = sums3[2] = 0.0;
    if (int_da < 2) return SPFM_OK;
    // Tile records live for one window of kIntWindow tiles (a multiple of the run length) and are
    // combined into one record per run of kIntRun tiles right away; the runs are then combined
    // level by level.  The tree depends on the tile count alone, not on the launch partition.
    const int64_t ntile = (int64_t)int_T * (int_T + 1) / 2;
    const int64_t n1 = (ntile + kIntRun - 1) / kIntRun;
    HIPC(int_rec.alloc(sizeof(IntRec) * (size_t)std::min<int64_t>(ntile, kIntWindow)));
    HIPC(int_rec2.alloc(sizeof(IntRec) * (size_t)(n1 + (n1 + kIntRun - 1) / kIntRun + 2)));
    IntRec* lvl[2] = {int_rec2.as<IntRec>(), int_rec2.as<IntRec>() + n1};
    IntArgs a = interaction_args();
    a.tol = tol;
    int_launches = 0;
    for (int64_t w0 = 0; w0 < ntile; w0 += kIntWindow) {
        const int64_t w1 = std::min<int64_t>(ntile, w0 + kIntWindow);
        a.rec = int_rec.as<IntRec>();
        a.rec_base = w0;
        rc = interaction_tiles<INT_STATS>(a, w0, w1);
        if (rc) return rc;
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
    rc = sync();
    if (rc) return rc;
    counts2[0] = out.cnt;
    sums3[0] = out.sumsq;
    sums3[1] = out.sumabs;
    sums3[2] = out.maxabs;
    return SPFM_OK;
}

// INT_EMIT into int_keys / int_vals (capacity `cap`); *n_found = pairs that qualified
int spfm_engine::interaction_emit(double tol, unsigned long long thr_key, int64_t cap,
                                  int64_t* n_found) {
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
    int rc = interaction_tiles<INT_EMIT>(a);
    if (rc) return rc;
    uint64_t found = 0;
    SPFM_TRY(download(&found, int_cnt.p, 1));
    rc = sync();
    if (rc) return rc;
    *n_found = (int64_t)found;
    return SPFM_OK;
}

int spfm_engine::interaction_topk(int order_idx, int64_t K, int32_t* rows, int32_t* cols,
                                  double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction_topk: n_out is NULL");
    *n_out = 0;
    if (K < 0) FAIL(SPFM_ERR_INVALID, "interaction_topk: K must be >= 0");
    if (K > ((int64_t)1 << 28)) FAIL(SPFM_ERR_UNSUPPORTED, "interaction_topk: K must be <= 2^28");
    if (K > 0 && (!rows || !cols || !vals)) FAIL(SPFM_ERR_INVALID, "interaction_topk: NULL output");
    int rc = interaction_prepare("interaction_topk", order_idx);
    if (rc) return rc;
    if (K == 0 || int_da < 2) return SPFM_OK;
    // Radix select on the f64 pattern of |W| (monotone once the sign is dropped): per level a
    // histogram of the next bits among the pairs whose higher bits equal the prefix found so far;
    // the bin whose tail first holds K pairs extends the prefix.  Counts are exact, so the size of
    // the candidate set is known before it is emitted.
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
        rc = interaction_tiles<INT_HIST>(a);
        if (rc) return rc;
        SPFM_TRY(download(hh.data(), int_hist.p, hh.size()));
        rc = sync();
        if (rc) return rc;
        int64_t cum = 0;
        int b = (1 << bits[L]) - 1;
        for (; b >= 0; --b) {
            cum += (int64_t)hh[(size_t)b];
            if (above + cum >= K) break;
        }
        if (b < 0) {  // (first level only) fewer than K non-zero pairs: all of them
            thr_key = 0;
            tail = above + cum;
            break;
        }
        prefix = (prefix << bits[L]) | (unsigned long long)b;
        thr_key = prefix << shifts[L];
        tail = above + cum;
        above += cum - (int64_t)hh[(size_t)b];
        prefix_shift = shifts[L];
        if (tail <= soft) break;
    }
    if (tail == 0) return SPFM_OK;
    if (tail > hard) {
        char buf[160];
        snprintf(buf, sizeof buf,
                 "interaction_topk: %lld pairs tie with the K-th magnitude (candidate bound %lld)",
                 (long long)tail, (long long)hard);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    int64_t found = 0;
    rc = interaction_emit(0.0, thr_key, tail, &found);
    if (rc) return rc;
    if (found != tail) FAIL(SPFM_ERR_RUNTIME, "interaction_topk: candidate count mismatch");
    std::vector<uint64_t> hk((size_t)tail);
    std::vector<double> hv((size_t)tail);
    SPFM_TRY(download(hk.data(), int_keys.p, hk.size()));
    SPFM_TRY(download(hv.data(), int_vals.p, hv.size()));
    rc = sync();
    if (rc) return rc;
    std::vector<int64_t> idx((size_t)tail);
    for (int64_t i = 0; i < tail; ++i) idx[(size_t)i] = i;
    const int64_t nk = std::min<int64_t>(K, tail);
    // |W| descending, then j, then j' ascending (the key is j << 32 | j')
    std::partial_sort(idx.begin(), idx.begin() + nk, idx.end(), [&](int64_t x, int64_t y) {
        const double ax = std::fabs(hv[(size_t)x]), ay = std::fabs(hv[(size_t)y]);
        if (ax != ay) return ax > ay;
        return hk[(size_t)x] < hk[(size_t)y];
    });
    for (int64_t i = 0; i < nk; ++i) {
        const uint64_t key = hk[(size_t)idx[(size_t)i]];
        rows[i] = (int32_t)(key >> 32);
        cols[i] = (int32_t)(key & 0xffffffffu);
        vals[i] = hv[(size_t)idx[(size_t)i]];
    }
    *n_out = nk;
    return SPFM_OK;
}

int spfm_engine::interaction_list(int order_idx, double tol, int64_t capacity, int32_t* rows,
                                  int32_t* cols, double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction_list: n_out is NULL");
    *n_out = 0;
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction_list: tol must be >= 0");
    if (capacity < 0) FAIL(SPFM_ERR_INVALID, "interaction_list: capacity must be >= 0");
    if (capacity > 0 && (!rows || !cols || !vals))
        FAIL(SPFM_ERR_INVALID, "interaction_list: NULL output");
    int rc = interaction_prepare("interaction_list", order_idx);
    if (rc) return rc;
    if (int_da < 2) return SPFM_OK;
    int64_t found = 0;
    rc = interaction_emit(tol, 0ull, capacity, &found);
    if (rc) return rc;
    *n_out = found;
    if (found > capacity) {
        char buf[160];
        snprintf(buf, sizeof buf, "interaction_list: %lld pairs above tol, capacity %lld",
                 (long long)found, (long long)capacity);
        FAIL(SPFM_ERR_INVALID, buf);
    }
    if (found == 0) return SPFM_OK;
    // sorted by (row, col) = by key: the emission order does not matter
    const size_t nf = (size_t)found;
    HIPC(int_keys2.alloc(sizeof(uint64_t) * nf));
    HIPC(int_vals2.alloc(sizeof(double) * nf));
    size_t temp_bytes = 0;
    HIPC(rocprim::radix_sort_pairs(nullptr, temp_bytes, int_keys.as<uint64_t>(),
                                   int_keys2.as<uint64_t>(), int_vals.as<double>(),
                                   int_vals2.as<double>(), nf, 0, 64, stream));
    HIPC(int_tmp.alloc(temp_bytes));
    HIPC(rocprim::radix_sort_pairs(int_tmp.p, temp_bytes, int_keys.as<uint64_t>(),
                                   int_keys2.as<uint64_t>(), int_vals.as<double>(),
                                   int_vals2.as<double>(), nf, 0, 64, stream));
    std::vector<uint64_t> hk(nf);
    SPFM_TRY(download(hk.data(), int_keys2.p, nf));
    SPFM_TRY(download(vals, int_vals2.p, nf));
    rc = sync();
    if (rc) return rc;
    for (size_t i = 0; i < nf; ++i) {
        rows[i] = (int32_t)(hk[i] >> 32);
        cols[i] = (int32_t)(hk[i] & 0xffffffffu);
    }
    return SPFM_OK;
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

}  // extern "C"
