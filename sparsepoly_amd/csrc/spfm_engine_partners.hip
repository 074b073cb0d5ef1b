// spfm_engine_partners.hip -- spfm_interaction_degrees / _partners (include/spfm.h): the
// per-feature views of W = P_o^T diag(lams) P_o.  For every feature, how many partners it has and
// how much weight they carry; for a list of features, the K strongest partners of each.  Both walk
// the full square of W on the pair unit's compaction and packed images (interaction_prepare,
// spfm_engine_interactions.hip): query rows in slabs against candidate strips, W consumed in
// registers, nothing of size d_a^2 allocated.  Read-only like the pair entries, and the scratch is
// part of the interaction scratch.  See DESIGN.md section 14b.
#include "spfm_engine.hip.h"
#include "spfm_partners.hip.h"

#include <algorithm>

static_assert(kPartMaxK == SPFM_INTERACTION_MAX_K, "header and device agree on the cap");
static_assert(PART_ABS == SPFM_PARTNERS_ABS && PART_POS == SPFM_PARTNERS_POS &&
                  PART_NEG == SPFM_PARTNERS_NEG,
              "header and device agree on the modes");

namespace {
constexpr int64_t kPartRecBytes = 256ll << 20;     // row records of one degree slab
constexpr int64_t kPartDegreeStrip = 16;           // tiles per strip of the degree pass
}  // namespace

int spfm_engine::interaction_degrees(int order_idx, double tol, int64_t cand_strip,
                                     int64_t* degree, double* sum_abs, double* max_abs,
                                     int32_t* strongest) {
    if (!(tol >= 0.0)) FAIL(SPFM_ERR_INVALID, "interaction_degrees: tol must be >= 0");
    if (cand_strip < 0 || cand_strip % kIntTile != 0)
        FAIL(SPFM_ERR_INVALID, "interaction_degrees: cand_strip must be 0 or a multiple of 64");
    SPFM_TRY(interaction_prepare("interaction_degrees", order_idx));
    int_launches = 0;
    // the caller's arrays are written only once nothing can fail
    std::vector<int64_t> hc((size_t)d, 0);
    std::vector<double> hs((size_t)d, 0.0), hm((size_t)d, 0.0);
    std::vector<int32_t> ha((size_t)d, -1);
    if (int_da >= 2) {
        const int da = int_da, T = int_T;
        const int64_t pad = (int64_t)T * kIntTile;
        const int strip_tiles = (int)std::min<int64_t>(
            T, cand_strip > 0 ? cand_strip / kIntTile : kPartDegreeStrip);
        const int n_strips = (int)cdiv(T, strip_tiles);
        int64_t slab = kPartRecBytes / ((int64_t)T * (int64_t)sizeof(PartRec)) / kIntTile * kIntTile;
        slab = std::min(std::max<int64_t>(slab, kIntTile), pad);
        HIPC(int_prec.alloc(sizeof(PartRec) * (size_t)slab * (size_t)T));
        // cnt, sum, mx (8 bytes each), arg (4) per padded compact rank
        HIPC(int_pdeg.alloc((size_t)pad * 28));
        PartOut out;
        out.cnt = int_pdeg.as<long long>();
        out.sum = reinterpret_cast<double*>(out.cnt + pad);
        out.mx = out.sum + pad;
        out.arg = reinterpret_cast<int32_t*>(out.mx + pad);
        const size_t lds = part_degree_lds_bytes();
        for (int64_t r0 = 0; r0 < pad; r0 += slab) {
            const int64_t rows_pad = std::min(slab, pad - r0);
            const int64_t nrow = std::min<int64_t>(rows_pad, da - r0);
            PartArgs a;
            memset(&a, 0, sizeof a);
            a.Q = int_A.as<double>() + (size_t)r0 * int_kp;
            a.B = int_B.as<double>();
            a.ids = int_ids.as<int32_t>();
            a.kp = int_kp;
            a.nrow = (int)nrow;
            a.rows_pad = (int)rows_pad;
            a.row0 = (int)r0;
            a.r_lo = 0;
            a.r_hi = da;
            a.t_lo = 0;
            a.t_hi = T;
            a.strip_tiles = strip_tiles;
            a.n_strips = n_strips;
            a.tol = tol;
            a.rec = int_prec.as<PartRec>();
            hipLaunchKernelGGL((part_tile_kernel<PART_DEGREE>),
                               dim3((unsigned)n_strips, (unsigned)(rows_pad / kIntTile)),
                               dim3(kBlock), lds, stream, a);
            hipLaunchKernelGGL(part_reduce_kernel, dim3(cdiv(nrow * kWave, kBlock)), dim3(kBlock),
                               0, stream, int_prec.as<PartRec>(), (int)nrow, T, (int)r0,
                               int_ids.as<int32_t>(), out);
            HIPC(hipGetLastError());
            ++int_launches;
        }
        std::vector<int32_t> ids((size_t)da), arg((size_t)da);
        std::vector<long long> cnt((size_t)da);
        std::vector<double> sum((size_t)da), mx((size_t)da);
        SPFM_TRY(download(ids.data(), int_ids.p, ids.size()));
        SPFM_TRY(download(cnt.data(), out.cnt, cnt.size()));
        SPFM_TRY(download(sum.data(), out.sum, sum.size()));
        SPFM_TRY(download(mx.data(), out.mx, mx.size()));
        SPFM_TRY(download(arg.data(), out.arg, arg.size()));
        SPFM_TRY(sync());
        for (int r = 0; r < da; ++r) {
            const int32_t j = ids[(size_t)r];
            if (j < 0 || j >= d) FAIL(SPFM_ERR_RUNTIME, "interaction_degrees: compaction failed");
            hc[(size_t)j] = cnt[(size_t)r];
            hs[(size_t)j] = sum[(size_t)r];
            hm[(size_t)j] = mx[(size_t)r];
            ha[(size_t)j] = arg[(size_t)r];
        }
    }
    if (degree) std::copy(hc.begin(), hc.end(), degree);
    if (sum_abs) std::copy(hs.begin(), hs.end(), sum_abs);
    if (max_abs) std::copy(hm.begin(), hm.end(), max_abs);
    if (strongest) std::copy(ha.begin(), ha.end(), strongest);
    return SPFM_OK;
}

int spfm_engine::interaction_partners(int order_idx, int64_t nJ, const int32_t* J, int64_t K,
                                      int32_t cand_lo, int32_t cand_hi, int by, int64_t row_slab,
                                      int64_t cand_strip, int32_t* ids_out, double* vals_out,
                                      int32_t* n_out) {
    BlockView v;
    SPFM_TRY(interaction_view("interaction_partners", order_idx, &v));
    if (K < 1) FAIL(SPFM_ERR_INVALID, "interaction_partners: K must be >= 1");
    if (K > SPFM_INTERACTION_MAX_K) {
        char buf[96];
        snprintf(buf, sizeof buf, "interaction_partners: K must be <= SPFM_INTERACTION_MAX_K = %d",
                 (int)SPFM_INTERACTION_MAX_K);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    if (by != SPFM_PARTNERS_ABS && by != SPFM_PARTNERS_POS && by != SPFM_PARTNERS_NEG)
        FAIL(SPFM_ERR_INVALID, "interaction_partners: by must be SPFM_PARTNERS_ABS, _POS or _NEG");
    if (row_slab < 0 || row_slab > (1 << 20))
        FAIL(SPFM_ERR_INVALID, "interaction_partners: row_slab must be in [0, 2^20]");
    if (cand_strip < 0 || cand_strip % kIntTile != 0 || cand_strip > kSelMaxStrip)
        FAIL(SPFM_ERR_INVALID,
             "interaction_partners: cand_strip must be 0 or a multiple of 64, at most 65536");
    const int dlim = (int_dlim > 0 && int_dlim < d) ? int_dlim : d;
    if (cand_lo < 0 || cand_hi > d)
        FAIL(SPFM_ERR_INVALID, "interaction_partners: candidate range outside [0, d]");
    const int hi = cand_hi <= 0 ? dlim : std::min<int>(cand_hi, dlim);
    if (cand_lo >= hi) FAIL(SPFM_ERR_INVALID, "interaction_partners: [cand_lo, cand_hi) is empty");
    if (J && nJ < 0) FAIL(SPFM_ERR_INVALID, "interaction_partners: negative size");
    const int64_t nq = J ? nJ : dlim;
    if (J)
        for (int64_t q = 0; q < nq; ++q)
            if (J[q] < 0 || J[q] >= d)
                FAIL(SPFM_ERR_INVALID, "interaction_partners: feature id out of range");
    if (nq > 0 && (!ids_out || !vals_out || !n_out))
        FAIL(SPFM_ERR_INVALID, "interaction_partners: NULL output");
    SPFM_TRY(interaction_prepare("interaction_partners", order_idx));
    int_launches = 0;
    if (nq == 0) return SPFM_OK;
    // the caller's arrays are written only once nothing can fail
    std::vector<int32_t> hi_((size_t)nq * K, -1), hn((size_t)nq, 0);
    std::vector<double> hv((size_t)nq * K, 0.0);
    int r_lo = 0, r_hi = 0;
    if (int_da >= 2) {
        std::vector<int32_t> ids((size_t)int_da);
        SPFM_TRY(download(ids.data(), int_ids.p, ids.size()));
        SPFM_TRY(sync());
        r_lo = (int)(std::lower_bound(ids.begin(), ids.end(), cand_lo) - ids.begin());
        r_hi = (int)(std::lower_bound(ids.begin(), ids.end(), hi) - ids.begin());
    }
    if (r_lo < r_hi) {
        const int t_lo = r_lo / kIntTile, t_hi = (int)cdiv(r_hi, kIntTile);
        const SelPlan plan = sel_plan(row_slab, cand_strip, nq, t_hi - t_lo);
        const int64_t slab = plan.slab;
        const int Ki = (int)K;
        HIPC(hipFuncSetAttribute((const void*)part_tile_kernel<PART_SELECT>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
        HIPC(int_pq.alloc(sizeof(double) * (size_t)slab * int_kp));
        HIPC(int_pqr.alloc(sizeof(int32_t) * (size_t)slab));
        HIPC(int_psel.alloc(plan.n_strips, slab, Ki));
        HIPC(int_pon.alloc(sizeof(int32_t) * (size_t)slab));
        if (J) SPFM_TRY(upload(int_io, J, (size_t)nq));
        for (int64_t r0 = 0; r0 < nq; r0 += slab) {
            const int64_t nrow = std::min(slab, nq - r0);
            const int64_t rows_pad = round_up(nrow, kIntTile);
            const int64_t total = rows_pad * int_kp;
            hipLaunchKernelGGL(part_gather_kernel, dim3(cdiv(total, kBlock)), dim3(kBlock), 0,
                               stream, int_A.as<double>(), int_kp, int_flag.as<int32_t>(),
                               int_pos.as<int32_t>(),
                               J ? int_io.as<int32_t>() + r0 : (const int32_t*)nullptr, (int)r0,
                               (int)nrow, total, int_pq.as<double>(), int_pqr.as<int32_t>());
            PartArgs a;
            memset(&a, 0, sizeof a);
            a.Q = int_pq.as<double>();
            a.B = int_B.as<double>();
            a.qrank = int_pqr.as<int32_t>();
            a.ids = int_ids.as<int32_t>();
            a.kp = int_kp;
            a.nrow = (int)nrow;
            a.rows_pad = (int)rows_pad;
            a.r_lo = r_lo;
            a.r_hi = r_hi;
            a.t_lo = t_lo;
            a.t_hi = t_hi;
            a.strip_tiles = plan.strip_tiles;
            a.n_strips = plan.n_strips;
            a.by = by;
            a.sel = {Ki, kSelCap, int_psel.lv.as<double>(), int_psel.li.as<int32_t>(),
                     int_psel.ov.as<double>(), int_psel.oi.as<int32_t>()};
            a.ocnt = int_pon.as<int32_t>();
            HIPC(int_psel.clear(nrow, Ki, 0, stream));  // slots no partner fills: id -1, value 0
            hipLaunchKernelGGL((part_tile_kernel<PART_SELECT>),
                               dim3((unsigned)plan.n_strips, (unsigned)(rows_pad / kIntTile)),
                               dim3(kBlock), plan.lds, stream, a);
            hipLaunchKernelGGL(part_merge_kernel, dim3(cdiv(nrow * kWave, kBlock)), dim3(kBlock), 0,
                               stream, a);
            HIPC(hipGetLastError());
            ++int_launches;
            SPFM_TRY(download(hv.data() + (size_t)r0 * Ki, int_psel.ov.p, (size_t)nrow * Ki));
            SPFM_TRY(download(hi_.data() + (size_t)r0 * Ki, int_psel.oi.p, (size_t)nrow * Ki));
            SPFM_TRY(download(hn.data() + (size_t)r0, int_pon.p, (size_t)nrow));
            SPFM_TRY(sync());  // the slab's buffers are rewritten by the next one
        }
    }
    std::copy(hi_.begin(), hi_.end(), ids_out);
    std::copy(hv.begin(), hv.end(), vals_out);
    std::copy(hn.begin(), hn.end(), n_out);
    return SPFM_OK;
}

extern "C" {

int spfm_interaction_degrees(spfm_handle h, int order_idx, double tol, int64_t cand_strip,
                             int64_t* degree, double* sum_abs, double* max_abs,
                             int32_t* strongest) {
    SPFM_GUARD(h);
    return h->interaction_degrees(order_idx, tol, cand_strip, degree, sum_abs, max_abs, strongest);
}

int spfm_interaction_partners(spfm_handle h, int order_idx, int64_t nJ, const int32_t* J,
                              int64_t K, int32_t cand_lo, int32_t cand_hi, int by,
                              int64_t row_slab, int64_t cand_strip, int32_t* ids, double* vals,
                              int32_t* n_out) {
    SPFM_GUARD(h);
    return h->interaction_partners(order_idx, nJ, J, K, cand_lo, cand_hi, by, row_slab, cand_strip,
                                   ids, vals, n_out);
}

}  // extern "C"
