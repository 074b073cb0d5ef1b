// spfm_engine_bank_auc.hip -- the host side of spfm_bank_group_auc and spfm_bank_group_curve
// (include/spfm.h; DESIGN.md sections 22 and 23): the checks beyond bank_check and the call's
// scratch, the keys of every slab behind bank_run's predict launches (spfm_engine_bank.hip drives
// the slabs and owns the C entries), and after the last slab one stable radix sort per member and
// the walks (spfm_bank_rank.hip.h from the bottom up, spfm_bank_curve.hip.h from the top down) on
// the same sorted copies, the members in batches that bound the sort buffers.
// The curve call's scratch is the AUC call's plus 8 kCurveRec = 96 bytes per (block, set, member of
// a batch) of its own block records, counted inside SPFM_BANK_AUC_MAX_BYTES:
//   9 n F + 4 n (+ 8 n weighted) + (12 n + (40 + 96) nb U) Fb + the sort's storage.
#include "spfm_engine.hip.h"
#include "spfm_bank_curve.hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <rocprim/device/device_radix_sort.hpp>

static_assert(kBankMaxSets == SPFM_BANK_MAX_SETS && kRankBlock == SPFM_BANK_RANK_BLOCK &&
                  kRankMaxModels == SPFM_BANK_MAX_MODELS,
              "header and device agree on the caps and on the block of the walk");
static_assert(SPFM_BANK_MAX_SETS <= kRankThreads, "one set per lane of the walk's wavefront");
static_assert(SPFM_BANK_MAX_GROUPS <= 32, "a set is a 32-bit mask; the group id takes 5 bits of meta");
static_assert(SPFM_BANK_CURVE_VALUES == 11 && SPFM_BANK_CURVE_COUNTS == 6,
              "curve_cell and auc_empty write the header's eleven values and six counts");

namespace {
// the sorted keys and rows of one batch of members: 12 n bytes per member
constexpr int64_t kAucBatchBytes = 128ll << 20;

int auc_batch(int64_t n, int F) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(F, kAucBatchBytes / (12 * std::max<int64_t>(n, 1))));
}

// the finite double behind a key of rank_key_dev; the key of both zeros gives +0.0
double auc_unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    double s;
    memcpy(&s, &b, sizeof s);
    return s;
}

hipError_t auc_sort(void* tmp, size_t& bytes, const uint64_t* kin, uint64_t* kout,
                    const uint32_t* vin, uint32_t* vout, int64_t n, hipStream_t stream) {
    return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, (size_t)n, 0u, 64u, stream);
}
}  // namespace

// U of the call: with sets NULL one set per group
static inline int auc_sets(const spfm_engine::BankCall& c) { return c.sets ? c.U : c.G; }

int spfm_engine::auc_check(const char* what, const BankCall& c) {
    const std::string w(what);
    char buf[200];
    const int F = bk_F;
    if (c.sets && c.U < 1) FAIL(SPFM_ERR_INVALID, w + ": U must be >= 1");
    if (c.sets && c.U > SPFM_BANK_MAX_SETS) {
        snprintf(buf, sizeof buf, "%s: %d sets exceed SPFM_BANK_MAX_SETS = %d", what, c.U,
                 (int)SPFM_BANK_MAX_SETS);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    if (c.sets && c.G < 32)
        for (int64_t s = 0; s < (int64_t)F * c.U; ++s)
            if (c.sets[s] >> c.G) {
                snprintf(buf, sizeof buf, "%s: set %d of member %d names a group at or above G = %d",
                         what, (int)(s % c.U), (int)(s / c.U), c.G);
                FAIL(SPFM_ERR_INVALID, buf);
            }
    const int U = auc_sets(c);
    const int64_t n = c.n, nb = (n + kRankBlock - 1) / kRankBlock;
    bk_abatch = auc_batch(n, F);
    if (const char* env = std::getenv("SPFM_BANK_AUC_BATCH"))  // test hook: smaller batches
        if (atoi(env) >= 1) bk_abatch = std::min(bk_abatch, atoi(env));
    int64_t need = 9 * n * F + 4 * n + (c.weight ? 8 * n : 0) + 12 * n * bk_abatch +
                   8 * kRankRec * nb * U * bk_abatch +
                   (c.curve ? 8 * kCurveRec * nb * U * bk_abatch : 0);
    bk_atmp_bytes = 0;
    if (need <= SPFM_BANK_AUC_MAX_BYTES && n > 0) {
        size_t tb = 0;  // (a query: rocPRIM touches no device here)
        HIPC(auc_sort(nullptr, tb, nullptr, nullptr, nullptr, nullptr, n, stream));
        bk_atmp_bytes = tb;
        need += (int64_t)tb;
    }
    if (need > SPFM_BANK_AUC_MAX_BYTES) {
        snprintf(buf, sizeof buf,
                 "%s: the resident scratch of %lld rows x %d members x %d sets is %lld bytes, above "
                 "SPFM_BANK_AUC_MAX_BYTES = %lld",
                 what, (long long)n, F, U, (long long)need, (long long)SPFM_BANK_AUC_MAX_BYTES);
        FAIL(SPFM_ERR_UNSUPPORTED, buf);
    }
    return SPFM_OK;
}

// n = 0 (or a table nobody walked): NaN and zeros
void spfm_engine::auc_empty(const BankCall& c) {
    const size_t cells = (size_t)bk_F * auc_sets(c);
    if (c.curve) {
        const int V = SPFM_BANK_CURVE_VALUES;
        for (size_t s = 0; s < cells; ++s) {
            std::fill(c.curve + V * s, c.curve + V * (s + 1), 0.0);
            for (int k : {0, 1, 2, 5, 6}) c.curve[V * s + k] = NAN;  // the values and thresholds
        }
        if (c.counts && !c.weight)
            std::fill(c.counts, c.counts + SPFM_BANK_CURVE_COUNTS * cells, (int64_t)0);
        if (!c.out) return;
    }
    for (size_t s = 0; s < cells; ++s) {
        c.out[3 * s] = NAN;
        c.out[3 * s + 1] = c.out[3 * s + 2] = 0.0;
    }
    if (c.pairs && !c.weight) std::fill(c.pairs, c.pairs + 3 * cells, (int64_t)0);
}

// the call's scratch goes when the call returns (bank_run), whatever it returns
void spfm_engine::auc_release() {
    for (DevBuf* b : {&bk_akey, &bk_ameta, &bk_arow, &bk_aw, &bk_askey, &bk_asrow, &bk_atmp,
                      &bk_asets, &bk_ablk, &bk_aout, &bk_cblk, &bk_cout})
        b->release();
}

int spfm_engine::auc_begin(const BankCall& c) {
    const int F = bk_F, U = auc_sets(c), Fb = bk_abatch;
    const size_t n = (size_t)c.n, nb = (n + kRankBlock - 1) / kRankBlock;
    HIPC(bk_akey.alloc(sizeof(uint64_t) * n * F));
    HIPC(bk_ameta.alloc(n * F));
    HIPC(bk_arow.alloc(sizeof(uint32_t) * n));
    if (c.weight) HIPC(bk_aw.alloc(sizeof(double) * n));
    HIPC(bk_askey.alloc(sizeof(uint64_t) * n * Fb));
    HIPC(bk_asrow.alloc(sizeof(uint32_t) * n * Fb));
    HIPC(bk_atmp.alloc(std::max<size_t>(bk_atmp_bytes, 16)));
    HIPC(bk_asets.alloc(sizeof(uint32_t) * (size_t)F * U));
    HIPC(bk_ablk.alloc(8 * (size_t)kRankRec * nb * U * Fb));
    HIPC(bk_aout.alloc(8 * (size_t)3 * U * Fb));
    if (c.curve) {
        HIPC(bk_cblk.alloc(8 * (size_t)kCurveRec * nb * U * Fb));
        HIPC(bk_cout.alloc(8 * (size_t)kCurveRes * U * Fb));
    }
    std::vector<uint32_t> own;  // staging of the default sets: set u = {u} for every member
    if (!c.sets) {
        own.resize((size_t)F * U);
        for (size_t s = 0; s < own.size(); ++s) own[s] = 1u << (s % U);
    }
    return run_staged([&]() -> int {
        SPFM_TRY(upload_to(bk_asets.p, c.sets ? c.sets : own.data(), (size_t)F * U));
        if (c.weight) SPFM_TRY(upload_to(bk_aw.p, c.weight, n));
        hipLaunchKernelGGL(bank_rank_iota_kernel, dim3(cdiv(c.n, kBlock)), dim3(kBlock), 0, stream,
                           c.n, bk_arow.as<uint32_t>());
        HIPC(hipGetLastError());
        return SPFM_OK;
    });
}

// behind the slab's predict launches: bk_sc, bk_y and bk_gg hold the slab
void spfm_engine::auc_slab(const BankCall& c, int64_t r0, int64_t rows) {
    const int F = bk_F;
    hipLaunchKernelGGL(bank_rank_key_kernel, dim3(cdiv(rows, kRankTile)), dim3(kBlock), 0, stream,
                       rows, r0, c.n, F, bk_sc.as<double>(), bk_y.as<double>(), c.per_model ? F : 1,
                       c.per_model ? 1 : 0, c.group ? bk_gg.as<int32_t>() : (const int32_t*)nullptr,
                       bk_akey.as<uint64_t>(), bk_ameta.as<uint8_t>());
}

template <typename A>
static void auc_walk(spfm_engine* e, int64_t n, int64_t nb, int U, int f0, int fb) {
    const uint64_t* sk = e->bk_askey.as<uint64_t>();
    const uint32_t* sr = e->bk_asrow.as<uint32_t>();
    const uint8_t* meta = e->bk_ameta.as<uint8_t>() + (size_t)f0 * n;
    const double* wt = e->bk_aw.as<double>();
    const uint32_t* sets = e->bk_asets.as<uint32_t>() + (size_t)f0 * U;
    A* rec = e->bk_ablk.as<A>();
    A* res = e->bk_aout.as<A>();
    const int cells = fb * U;
    const dim3 grid((unsigned)nb, (unsigned)fb);
    hipLaunchKernelGGL((bank_rank_block_kernel<A>), grid, dim3(kRankThreads), 0, e->stream, n, nb, U,
                       sk, sr, meta, wt, sets, rec);
    hipLaunchKernelGGL((bank_rank_carry_kernel<A>), dim3(cdiv(cells, kBlock)), dim3(kBlock), 0,
                       e->stream, nb, cells, 0, rec, res);
    hipLaunchKernelGGL((bank_rank_finish_kernel<A>), grid, dim3(kRankThreads), 0, e->stream, n, nb, U,
                       sk, sr, meta, wt, sets, rec);
    hipLaunchKernelGGL((bank_rank_carry_kernel<A>), dim3(cdiv(cells, kBlock)), dim3(kBlock), 0,
                       e->stream, nb, cells, 1, rec, res);
}

template <typename A>
static void curve_walk(spfm_engine* e, int64_t n, int64_t nb, int U, int f0, int fb) {
    const uint64_t* sk = e->bk_askey.as<uint64_t>();
    const uint32_t* sr = e->bk_asrow.as<uint32_t>();
    const uint8_t* meta = e->bk_ameta.as<uint8_t>() + (size_t)f0 * n;
    const double* wt = e->bk_aw.as<double>();
    const uint32_t* sets = e->bk_asets.as<uint32_t>() + (size_t)f0 * U;
    CurveRec<A>* rec = e->bk_cblk.as<CurveRec<A>>();
    CurveRes<A>* res = e->bk_cout.as<CurveRes<A>>();
    const int cells = fb * U;
    const dim3 grid((unsigned)nb, (unsigned)fb);
    hipLaunchKernelGGL((bank_curve_block_kernel<A>), grid, dim3(kRankThreads), 0, e->stream, n, nb,
                       U, sk, sr, meta, wt, sets, rec);
    hipLaunchKernelGGL((bank_curve_carry_kernel<A>), dim3(cdiv(cells, kBlock)), dim3(kBlock), 0,
                       e->stream, n, nb, U, cells, 0, sk, rec, res);
    hipLaunchKernelGGL((bank_curve_finish_kernel<A>), grid, dim3(kRankThreads), 0, e->stream, n, nb,
                       U, sk, sr, meta, wt, sets, rec, res);
    hipLaunchKernelGGL((bank_curve_carry_kernel<A>), dim3(cdiv(cells, kBlock)), dim3(kBlock), 0,
                       e->stream, n, nb, U, cells, 1, sk, rec, res);
}

// one (member, set) of the curve's table from the device's result: the quotients are formed here,
// once, in the stated form; what is undefined is NaN with TP = FP = 0
template <typename A>
static void curve_cell(const int64_t* raw, double* o, int64_t* counts) {
    CurveRes<A> r;
    memcpy(&r, raw, sizeof r);
    const double wpos = (double)r.wpos, wneg = (double)r.wneg;
    std::fill(o, o + SPFM_BANK_CURVE_VALUES, 0.0);
    o[0] = o[1] = o[2] = o[5] = o[6] = NAN;
    o[9] = wpos;
    o[10] = wneg;
    const bool f1 = r.wpos > 0 && r.f1_pos >= 0, ks = r.wpos > 0 && r.wneg > 0 && r.ks_pos >= 0;
    if (r.wpos > 0) o[0] = r.ap / wpos;
    if (f1) {
        if constexpr (std::is_same<A, double>::value)
            o[1] = 2.0 * r.f1_tp / ((r.f1_tp + r.f1_fp) + r.wpos);
        else
            o[1] = (double)(2 * r.f1_tp) / (double)(r.f1_tp + r.f1_fp + r.wpos);
        o[2] = auc_unkey(r.f1_key);
        o[3] = (double)r.f1_tp;
        o[4] = (double)r.f1_fp;
    }
    if (ks) {
        if constexpr (std::is_same<A, double>::value) {
            // (the integer form in doubles: integer weights give the bits of replicated rows)
            o[5] = std::fabs(r.ks_tp * r.wneg - r.ks_fp * r.wpos) / (r.wpos * r.wneg);
        } else {
            const int64_t v = r.ks_tp * r.wneg - r.ks_fp * r.wpos;
            o[5] = (double)(v < 0 ? -v : v) / (wpos * wneg);
        }
        o[6] = auc_unkey(r.ks_key);
        o[7] = (double)r.ks_tp;
        o[8] = (double)r.ks_fp;
    }
    if constexpr (std::is_same<A, int64_t>::value)
        if (counts) {
            counts[0] = r.wpos;
            counts[1] = r.wneg;
            counts[2] = f1 ? r.f1_tp : 0;
            counts[3] = f1 ? r.f1_fp : 0;
            counts[4] = ks ? r.ks_tp : 0;
            counts[5] = ks ? r.ks_fp : 0;
        }
}

// after the last slab: batch after batch the members' sorts, the walks and the batch's results
int spfm_engine::auc_finish(const BankCall& c) {
    const int F = bk_F, U = auc_sets(c), Fb = bk_abatch;
    const int64_t n = c.n, nb = (n + kRankBlock - 1) / kRankBlock;
    static_assert(sizeof(int64_t) == sizeof(double), "one result buffer for both instantiations");
    std::vector<int64_t> raw((size_t)std::max(3, c.curve ? kCurveRes : 0) * U * Fb);
    for (int f0 = 0; f0 < F; f0 += Fb) {
        const int fb = std::min(Fb, F - f0);
        for (int f = 0; f < fb; ++f) {
            size_t tb = bk_atmp_bytes;
            HIPC(auc_sort(bk_atmp.p, tb, bk_akey.as<uint64_t>() + (size_t)(f0 + f) * n,
                          bk_askey.as<uint64_t>() + (size_t)f * n, bk_arow.as<uint32_t>(),
                          bk_asrow.as<uint32_t>() + (size_t)f * n, n, stream));
        }
        if (c.curve) {  // its walk on the same sorted copies; the AUC walk below only where asked
            if (c.weight)
                curve_walk<double>(this, n, nb, U, f0, fb);
            else
                curve_walk<int64_t>(this, n, nb, U, f0, fb);
            HIPC(hipGetLastError());
            SPFM_TRY(download(raw.data(), bk_cout.p, (size_t)kCurveRes * U * fb));
            SPFM_TRY(sync());
            for (int s = 0; s < fb * U; ++s) {
                const size_t cell = (size_t)f0 * U + s;
                double* o = c.curve + SPFM_BANK_CURVE_VALUES * cell;
                if (c.weight)
                    curve_cell<double>(&raw[(size_t)kCurveRes * s], o, nullptr);
                else
                    curve_cell<int64_t>(&raw[(size_t)kCurveRes * s], o,
                                        c.counts ? c.counts + SPFM_BANK_CURVE_COUNTS * cell : nullptr);
            }
            if (!c.out) continue;
        }
        if (c.weight)
            auc_walk<double>(this, n, nb, U, f0, fb);
        else
            auc_walk<int64_t>(this, n, nb, U, f0, fb);
        HIPC(hipGetLastError());
        SPFM_TRY(download(raw.data(), bk_aout.p, (size_t)3 * U * fb));
        SPFM_TRY(sync());
        for (int s = 0; s < fb * U; ++s) {
            double* o = c.out + 3 * ((size_t)f0 * U + s);
            if (c.weight) {
                double v[3];
                memcpy(v, &raw[3 * (size_t)s], sizeof v);
                o[0] = v[1] * v[2] > 0.0 ? 0.5 * v[0] / (v[1] * v[2]) : NAN;
                o[1] = v[1];
                o[2] = v[2];
            } else {
                const int64_t* v = &raw[3 * (size_t)s];
                o[0] = (v[1] > 0 && v[2] > 0) ? (double)v[0] / (2.0 * (double)v[1] * (double)v[2]) : NAN;
                o[1] = (double)v[1];
                o[2] = (double)v[2];
                if (c.pairs) std::copy(v, v + 3, c.pairs + 3 * ((size_t)f0 * U + s));
            }
        }
    }
    return SPFM_OK;
}
