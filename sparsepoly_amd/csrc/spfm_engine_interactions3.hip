// spfm_engine_interactions3.hip -- spfm_interaction3_stats / _topk / _list / _values
// (include/spfm.h): which feature TRIPLES the model kept, from the live device parameters.
// T[a, j, l] = sum_s lams_s p_sa p_sj p_sl over a < j < l is formed in registers, pivot by pivot
// on the 64 x 64 tiles of the pair pass, and consumed there; nothing of size d_a^3 or d_a^2 is
// allocated.  Compaction, packed images and every scratch buffer are those of the pair unit
// (spfm_engine_interactions.hip): read-only in the same sense, freed by the same three things.
// See DESIGN.md section 14a.
#include "spfm_engine.hip.h"
#include "spfm_interactions3.hip.h"
#include "spfm_interactions3_host.h"

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>

static_assert(kInt3KeyBits == kInt3IdBits, "host and device agree on the key");

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

// the units [u0, u1), at most `interaction_tile_budget` of them per launch
template <int MODE>
int spfm_engine::interaction3_units(Int3Args a, int64_t u0, int64_t u1) {
    const int64_t per = int_tile_budget > 0 ? int_tile_budget : kInt3Window;
    for (; u0 < u1; u0 += per) {
        a.p.tile0 = u0;
        const int64_t nu = std::min<int64_t>(per, u1 - u0);
        hipLaunchKernelGGL((int3_tile_kernel<MODE>), dim3((unsigned)nu), dim3(kBlock), 0, stream, a);
        ++int_launches;
    }
    HIPC(hipGetLastError());
    return SPFM_OK;
}

template <int MODE>
int spfm_engine::interaction3_units(Int3Args a) {
    int_launches = 0;
    return interaction3_units<MODE>(a, 0, int3_units_before(int_T, int_T));
}

int spfm_engine::interaction3_stats(int order_idx, double tol, int64_t* counts2, double* sums3) {
    if (!counts2 || !sums3) FAIL(SPFM_ERR_INVALID, "interaction3_stats: NULL output");
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction3_stats: tol must be >= 0");
    int rc = interaction3_prepare("interaction3_stats", order_idx);
    if (rc) return rc;
    counts2[0] = 0;
    counts2[1] = int_da;
    sums3[0] = sums3[1] = sums3[2] = 0.0;
    if (int_da < 3) return SPFM_OK;
    // As the pair pass: unit records live for one window (a multiple of the run length) and are
    // combined into one record per run of kIntRun units right away; the runs are then combined
    // level by level.  The tree depends on the unit count alone, not on the launch partition.
    const int64_t nunit = int3_units_before(int_T, int_T);
    const int64_t n1 = (nunit + kIntRun - 1) / kIntRun;
    HIPC(int_rec.alloc(sizeof(IntRec) * (size_t)std::min<int64_t>(nunit, kInt3Window)));
    HIPC(int_rec2.alloc(sizeof(IntRec) * (size_t)(n1 + (n1 + kIntRun - 1) / kIntRun + 2)));
    IntRec* lvl[2] = {int_rec2.as<IntRec>(), int_rec2.as<IntRec>() + n1};
    Int3Args a{interaction_args(), int_da};
    a.p.tol = tol;
    int_launches = 0;
    for (int64_t w0 = 0; w0 < nunit; w0 += kInt3Window) {
        const int64_t w1 = std::min<int64_t>(nunit, w0 + kInt3Window);
        a.p.rec = int_rec.as<IntRec>();
        a.p.rec_base = w0;
        rc = interaction3_units<INT_STATS>(a, w0, w1);
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

// INT_EMIT into int_keys / int_vals (capacity `cap`); *n_found = triples that qualified
int spfm_engine::interaction3_emit(double tol, unsigned long long thr_key, int64_t cap,
                                   int64_t* n_found) {
    HIPC(int_keys.alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(cap, 1)));
    HIPC(int_vals.alloc(sizeof(double) * (size_t)std::max<int64_t>(cap, 1)));
    HIPC(int_cnt.alloc(sizeof(uint64_t)));
    HIPC(hipMemsetAsync(int_cnt.p, 0, sizeof(uint64_t), stream));
    Int3Args a{interaction_args(), int_da};
    a.p.tol = tol;
    a.p.thr_key = thr_key;
    a.p.cap = (unsigned long long)cap;
    a.p.counter = int_cnt.as<unsigned long long>();
    a.p.keys = int_keys.as<unsigned long long>();
    a.p.vals = int_vals.as<double>();
    int rc = interaction3_units<INT_EMIT>(a);
    if (rc) return rc;
    uint64_t found = 0;
    SPFM_TRY(download(&found, int_cnt.p, 1));
    rc = sync();
    if (rc) return rc;
    *n_found = (int64_t)found;
    return SPFM_OK;
}

// keys of compacted ids -> feature ids (int_ids of the last compaction)
int spfm_engine::interaction3_unpack(const uint64_t* keys, size_t n, int32_t* i, int32_t* j,
                                     int32_t* l) {
    std::vector<int32_t> ids((size_t)int_da);
    SPFM_TRY(download(ids.data(), int_ids.p, ids.size()));
    SPFM_TRY(sync());
    for (size_t q = 0; q < n; ++q)
        if (!int3_unpack_key(keys[q], ids.data(), int_da, i + q, j + q, l + q))
            FAIL(SPFM_ERR_RUNTIME, "interaction3: emitted id out of range");
    return SPFM_OK;
}

int spfm_engine::interaction3_topk(int order_idx, int64_t K, int32_t* i, int32_t* j, int32_t* l,
                                   double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction3_topk: n_out is NULL");
    *n_out = 0;
    if (K < 0) FAIL(SPFM_ERR_INVALID, "interaction3_topk: K must be >= 0");
    if (K > ((int64_t)1 << 28)) FAIL(SPFM_ERR_UNSUPPORTED, "interaction3_topk: K must be <= 2^28");
    if (K > 0 && (!i || !j || !l || !vals)) FAIL(SPFM_ERR_INVALID, "interaction3_topk: NULL output");
    int rc = interaction3_prepare("interaction3_topk", order_idx);
    if (rc) return rc;
    if (K == 0 || int_da < 3) return SPFM_OK;
    // The radix select of the pair pass on the f64 pattern of |T|: per level a histogram of the
    // next bits among the triples whose higher bits equal the prefix found so far; the bin whose
    // tail first holds K triples extends the prefix.  Counts are exact, so the size of the
    // candidate set is known before it is emitted.
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
        Int3Args a{interaction_args(), int_da};
        a.p.hist = int_hist.as<unsigned long long>();
        a.p.prefix = prefix;
        a.p.prefix_shift = prefix_shift;
        a.p.bin_shift = shifts[L];
        a.p.bin_mask = (1u << bits[L]) - 1u;
        rc = interaction3_units<INT_HIST>(a);
        if (rc) return rc;
        SPFM_TRY(download(hh.data(), int_hist.p, hh.size()));
        rc = sync();
        if (rc) return rc;
        int64_t above_next = 0;
        const int b = int3_select_bin(hh.data(), 1 << bits[L], above, K, &tail, &above_next);
        if (b < 0) {  // (first level only) fewer than K non-zero triples: all of them
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
                 "interaction3_topk: %lld triples tie with the K-th magnitude (candidate bound %lld)",
                 (long long)tail, (long long)hard);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    int64_t found = 0;
    rc = interaction3_emit(0.0, thr_key, tail, &found);
    if (rc) return rc;
    if (found != tail) FAIL(SPFM_ERR_RUNTIME, "interaction3_topk: candidate count mismatch");
    std::vector<uint64_t> hk((size_t)tail);
    std::vector<double> hv((size_t)tail);
    SPFM_TRY(download(hk.data(), int_keys.p, hk.size()));
    SPFM_TRY(download(hv.data(), int_vals.p, hv.size()));
    rc = sync();
    if (rc) return rc;
    // |T| descending, then i, j, l ascending (the key orders the compacted ids, compaction is
    // monotone)
    std::vector<int64_t> idx;
    const int64_t nk = int3_order_candidates(hk, hv, K, idx);
    std::vector<uint64_t> top((size_t)nk);
    for (int64_t q = 0; q < nk; ++q) {
        top[(size_t)q] = hk[(size_t)idx[(size_t)q]];
        vals[q] = hv[(size_t)idx[(size_t)q]];
    }
    SPFM_TRY(interaction3_unpack(top.data(), top.size(), i, j, l));
    *n_out = nk;
    return SPFM_OK;
}

int spfm_engine::interaction3_list(int order_idx, double tol, int64_t capacity, int32_t* i,
                                   int32_t* j, int32_t* l, double* vals, int64_t* n_out) {
    if (!n_out) FAIL(SPFM_ERR_INVALID, "interaction3_list: n_out is NULL");
    *n_out = 0;
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction3_list: tol must be >= 0");
    if (capacity < 0) FAIL(SPFM_ERR_INVALID, "interaction3_list: capacity must be >= 0");
    if (capacity > 0 && (!i || !j || !l || !vals))
        FAIL(SPFM_ERR_INVALID, "interaction3_list: NULL output");
    int rc = interaction3_prepare("interaction3_list", order_idx);
    if (rc) return rc;
    if (int_da < 3) return SPFM_OK;
    int64_t found = 0;
    rc = interaction3_emit(tol, 0ull, capacity, &found);
    if (rc) return rc;
    *n_out = found;
    if (found > capacity) {
        char buf[160];
        snprintf(buf, sizeof buf, "interaction3_list: %lld triples above tol, capacity %lld",
                 (long long)found, (long long)capacity);
        FAIL(SPFM_ERR_INVALID, buf);
    }
    if (found == 0) return SPFM_OK;
    // sorted by (i, j, l) = by key: the emission order does not matter
    const size_t nf = (size_t)found;
    HIPC(int_keys2.alloc(sizeof(uint64_t) * nf));
    HIPC(int_vals2.alloc(sizeof(double) * nf));
    size_t temp_bytes = 0;
    HIPC(rocprim::radix_sort_pairs(nullptr, temp_bytes, int_keys.as<uint64_t>(),
                                   int_keys2.as<uint64_t>(), int_vals.as<double>(),
                                   int_vals2.as<double>(), nf, 0, 3 * kInt3IdBits, stream));
    HIPC(int_tmp.alloc(temp_bytes));
    HIPC(rocprim::radix_sort_pairs(int_tmp.p, temp_bytes, int_keys.as<uint64_t>(),
                                   int_keys2.as<uint64_t>(), int_vals.as<double>(),
                                   int_vals2.as<double>(), nf, 0, 3 * kInt3IdBits, stream));
    std::vector<uint64_t> hk(nf);
    std::vector<double> hv(nf);  // the caller's arrays are written only once nothing can fail
    SPFM_TRY(download(hk.data(), int_keys2.p, nf));
    SPFM_TRY(download(hv.data(), int_vals2.p, nf));
    rc = sync();
    if (rc) return rc;
    SPFM_TRY(interaction3_unpack(hk.data(), nf, i, j, l));
    std::copy(hv.begin(), hv.end(), vals);
    return SPFM_OK;
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
