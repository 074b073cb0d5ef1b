// spfm_engine_gram.hip -- Gram matrices and poly_predict of sparsepoly.kernels (kernels.py:51-153):
// spfm_gram_csr_dense / spfm_gram_csr_csr.  Kernels in spfm_gram.hip.h; DESIGN.md section
// "Gram matrices".
//
// The problem is cut into column tiles of the second operand (multiples of 64 columns) and row
// blocks of X so that the device buffers of one (tile, block) stay under the call's budget; each
// block of the result is copied into the caller's array as soon as it is done.  Every output
// element is computed by one lane in a fixed order and the K * lams partial sums of each
// 64-column chunk are folded in column order, so the result is the same for any budget.
#include "spfm_engine.hip.h"
#include "spfm_gram.hip.h"

using namespace spfm;

namespace {

constexpr int64_t kGramDefaultBudget = (int64_t)4 << 30;
constexpr int64_t kGramMaxRows = (int64_t)1 << 24;  // rows of one block (int in the kernels)

// one instantiation per kind and ANOVA capacity; any runtime degree up to the capacity
typedef void (*DenseLaunch)(const GramDenseArgs&, dim3, hipStream_t);
typedef void (*CsrLaunch)(const GramCsrArgs&, dim3, hipStream_t);

template <int KIND, int CAP>
void launch_dense(const GramDenseArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((gram_dense_kernel<KIND, CAP>), grid, dim3(kBlock), 0, s, a);
}
template <int KIND, int CAP>
void launch_csr(const GramCsrArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((gram_csr_kernel<KIND, CAP>), grid, dim3(kBlock), 0, s, a);
}

DenseLaunch pick_dense(int kind, int degree) {
    if (kind == GRAM_POLY) return launch_dense<GRAM_POLY, 1>;
    if (kind == GRAM_ALL_SUBSETS) return launch_dense<GRAM_ALL_SUBSETS, 1>;
    if (degree <= 2) return launch_dense<GRAM_ANOVA, 2>;
    if (degree <= 3) return launch_dense<GRAM_ANOVA, 3>;
    if (degree <= 4) return launch_dense<GRAM_ANOVA, 4>;
    if (degree <= 6) return launch_dense<GRAM_ANOVA, 6>;
    if (degree <= 8) return launch_dense<GRAM_ANOVA, 8>;
    if (degree <= 16) return launch_dense<GRAM_ANOVA, 16>;
    if (degree <= 32) return launch_dense<GRAM_ANOVA, 32>;
    return launch_dense<GRAM_ANOVA, 64>;
}

CsrLaunch pick_csr(int kind, int degree) {
    if (kind == GRAM_POLY) return launch_csr<GRAM_POLY, 1>;
    if (kind == GRAM_ALL_SUBSETS) return launch_csr<GRAM_ALL_SUBSETS, 1>;
    if (degree <= 2) return launch_csr<GRAM_ANOVA, 2>;
    if (degree <= 3) return launch_csr<GRAM_ANOVA, 3>;
    if (degree <= 4) return launch_csr<GRAM_ANOVA, 4>;
    if (degree <= 6) return launch_csr<GRAM_ANOVA, 6>;
    if (degree <= 8) return launch_csr<GRAM_ANOVA, 8>;
    if (degree <= 16) return launch_csr<GRAM_ANOVA, 16>;
    if (degree <= 32) return launch_csr<GRAM_ANOVA, 32>;
    return launch_csr<GRAM_ANOVA, 64>;
}

int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct GramRun {
    spfm_engine& eng;  // the handle: its stream, its typed copies, its error text
    std::string& err;
    hipStream_t stream;
    int kind, degree;
    const double* lams;
    int64_t budget;
    double* out;

    GramRun(spfm_engine& e, int kind_, int degree_, const double* lams_, int64_t budget_,
            double* out_)
        : eng(e), err(e.err), stream(e.stream), kind(kind_), degree(degree_), lams(lams_),
          budget(budget_), out(out_) {}

    // kind / degree of kernels.py; degree <= 1 of anova is X P^T (kernels.py:98-115 with an
    // empty recursion), i.e. the DP's a[1]
    int check_kind() {
        if (kind != SPFM_GRAM_ANOVA && kind != SPFM_GRAM_POLY && kind != SPFM_GRAM_ALL_SUBSETS)
            FAIL(SPFM_ERR_INVALID, "gram: unknown kernel kind");
        if (kind == SPFM_GRAM_ANOVA) {
            if (degree > SPFM_GRAM_MAX_DEGREE)
                FAIL(SPFM_ERR_UNSUPPORTED, "gram: anova degree above SPFM_GRAM_MAX_DEGREE (64)");
            if (degree < 1) degree = 1;
        }
        if (kind == SPFM_GRAM_POLY && degree < 0)
            FAIL(SPFM_ERR_UNSUPPORTED, "gram: poly kernel needs degree >= 0");
        if (!out) FAIL(SPFM_ERR_INVALID, "gram: out is NULL");
        if (budget < 0) FAIL(SPFM_ERR_INVALID, "gram: max_block_bytes < 0");
        if (budget == 0) {
            budget = kGramDefaultBudget;
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0)
                budget = std::min(budget, (int64_t)(fr / 2));
        }
        return SPFM_OK;
    }

    // indptr[n+1] from 0, nondecreasing; indices in [0, d), strictly increasing in each row
    int check_csr(const char* what, int64_t n, int32_t d, const int64_t* indptr,
                  const int32_t* indices, const double* data) {
        if (n < 0 || d < 0) FAIL(SPFM_ERR_INVALID, std::string("gram: negative shape of ") + what);
        if (!indptr) FAIL(SPFM_ERR_INVALID, std::string("gram: indptr of ") + what + " is NULL");
        if (indptr[0] != 0) FAIL(SPFM_ERR_INVALID, std::string("gram: indptr[0] != 0 in ") + what);
        for (int64_t r = 0; r < n; ++r) {
            const int64_t b = indptr[r], e = indptr[r + 1];
            if (e < b) FAIL(SPFM_ERR_INVALID, std::string("gram: indptr of ") + what +
                                                  " decreases");
            int64_t prev = -1;
            for (int64_t ii = b; ii < e; ++ii) {
                const int32_t c = indices[ii];
                if (c < 0 || c >= d)
                    FAIL(SPFM_ERR_INVALID, std::string("gram: column index out of range in ") +
                                               what);
                if (c <= prev)
                    FAIL(SPFM_ERR_INVALID, std::string("gram: indices of ") + what +
                                               " must be sorted and duplicate-free per row");
                prev = c;
            }
        }
        if (indptr[n] > 0 && (!indices || !data))
            FAIL(SPFM_ERR_INVALID, std::string("gram: entries of ") + what + " are NULL");
        return SPFM_OK;
    }

    // Row blocks [r0, r1) of X whose entries plus `per_row` output bytes fit `room`
    // (at least one row per block).
    static void row_blocks(int64_t n, const int64_t* indptr, int64_t per_row, int64_t room,
                           std::vector<int64_t>& bounds) {
        bounds.assign(1, 0);
        int64_t r0 = 0;
        while (r0 < n) {
            int64_t r = r0, bytes = 8;
            while (r < n && r - r0 < kGramMaxRows) {
                const int64_t rb = 8 + (indptr[r + 1] - indptr[r]) * 12 + per_row;
                if (r > r0 && bytes + rb > room) break;
                bytes += rb;
                ++r;
            }
            bounds.push_back(r);
            r0 = r;
        }
    }

    // lams: fold this block's chunk partials into out[r0..r1) in column order
    static void fold(const std::vector<double>& part, int64_t rows, int nch, bool first,
                     double* o) {
        for (int64_t r = 0; r < rows; ++r) {
            double acc = first ? 0.0 : o[r];
            for (int c = 0; c < nch; ++c) acc += part[(size_t)r * nch + c];
            o[r] = acc;
        }
    }

    int upload_rows(DevBuf& rp, DevBuf& ri, DevBuf& rv, const int64_t* indptr,
                    const int32_t* indices, const double* data, int64_t r0, int64_t r1) {
        std::vector<double> unused;  // double storage: no conversion, nothing staged
        return eng.stage_csr_rows(rp, ri, rv, unused, indptr, indices, data, r0, r1, 1);
    }

    // the K block of rows [r0, r0+rows) x columns [j0, j0+nt) into the caller's array
    int download_block(const DevBuf& o, int64_t n1, int64_t n2, int64_t r0, int64_t rows,
                       int64_t j0, int64_t nt, bool transpose_out) {
        if (transpose_out) {  // out is (n2 x n1); the block is (nt x rows)
            HIPC(hipMemcpy2DAsync(out + j0 * n1 + r0, sizeof(double) * (size_t)n1, o.p,
                                  sizeof(double) * (size_t)rows, sizeof(double) * (size_t)rows,
                                  (size_t)nt, hipMemcpyDeviceToHost, stream));
        } else if (nt == n2) {
            SPFM_TRY(eng.download(out + r0 * n2, o.p, (size_t)(rows * nt)));
        } else {
            HIPC(hipMemcpy2DAsync(out + r0 * n2 + j0, sizeof(double) * (size_t)n2, o.p,
                                  sizeof(double) * (size_t)nt, sizeof(double) * (size_t)nt,
                                  (size_t)rows, hipMemcpyDeviceToHost, stream));
        }
        return SPFM_OK;
    }

    int finish_lams_block(const DevBuf& o, int64_t r0, int64_t rows, int nch, int64_t nch_all,
                          bool first, std::vector<double>& hpart) {
        if (nch_all == 1) {  // one chunk in the whole call: the partial is the value
            return eng.download(out + r0, o.p, (size_t)rows);
        }
        hpart.resize((size_t)(rows * nch));
        SPFM_TRY(eng.download(hpart.data(), o.p, hpart.size()));
        HIPC(hipStreamSynchronize(stream));
        fold(hpart, rows, nch, first, out + r0);
        return SPFM_OK;
    }

    int empty_result(int64_t n1) {
        if (lams) std::memset(out, 0, sizeof(double) * (size_t)n1);
        return SPFM_OK;
    }

    // ------------------------------------------------------------ CSR x dense
    int csr_dense(int64_t n1, int32_t d, const int64_t* indptr, const int32_t* indices,
                  const double* data, int64_t n2, const double* B, int transpose_out) {
        int rc = check_kind();
        if (rc) return rc;
        if (n2 < 0 || n2 > INT32_MAX) FAIL(SPFM_ERR_INVALID, "gram: bad n2");
        if ((rc = check_csr("X", n1, d, indptr, indices, data))) return rc;
        if (!B && n2 > 0 && d > 0) FAIL(SPFM_ERR_INVALID, "gram: B is NULL");
        if (transpose_out && lams)
            FAIL(SPFM_ERR_INVALID, "gram: transpose_out applies to the Gram matrix only");
        if (n1 == 0 || n2 == 0) return empty_result(n1);
        // column tiles: multiples of 64 columns whose transposed image takes <= half the budget
        const int64_t col_bytes = std::max<int64_t>(1, (int64_t)d * 8);
        int64_t nt_max = std::max<int64_t>(1, (budget / 2) / (col_bytes * kGramChunk)) * kGramChunk;
        if (nt_max >= n2) nt_max = n2;
        const int64_t nch_all = cdiv64(n2, kGramChunk);
        DenseLaunch launch = pick_dense(kind, degree);
        DevBuf bt, rp, ri, rv, o, dl;
        std::vector<double> hbt, hpart;
        std::vector<int64_t> bounds;
        for (int64_t j0 = 0; j0 < n2; j0 += nt_max) {
            const int64_t nt = std::min(nt_max, n2 - j0);
            const int nch = (int)cdiv64(nt, kGramChunk);
            // the tile transposed: (d x nt), the nt values of one feature contiguous
            hbt.resize((size_t)std::max<int64_t>(1, (int64_t)d * nt));
            for (int64_t j = 0; j < nt; ++j) {
                const double* src = B + (j0 + j) * (int64_t)d;
                for (int32_t c = 0; c < d; ++c) hbt[(size_t)c * nt + j] = src[c];
            }
            HIPC(hipStreamSynchronize(stream));  // the previous tile's readers of bt are done
            SPFM_TRY(eng.upload(bt, hbt.data(), hbt.size()));
            if (lams) SPFM_TRY(eng.upload(dl, lams + j0, (size_t)nt));
            int group = 1;  // lanes per row: the next power of two >= nt, at most 64
            while (group < nt && group < kGramChunk) group <<= 1;
            const int cpw = nch >= 4 ? 4 : (nch >= 2 ? 2 : 1);
            const int rows_per_wg = (kBlock / group) / cpw;
            const int64_t per_row = lams ? (int64_t)nch * 8 : nt * 8;
            const int64_t room = std::max<int64_t>(budget - (int64_t)hbt.size() * 8, 1);
            row_blocks(n1, indptr, per_row, room, bounds);
            for (size_t bi = 0; bi + 1 < bounds.size(); ++bi) {
                const int64_t r0 = bounds[bi], r1 = bounds[bi + 1], rows = r1 - r0;
                if ((rc = upload_rows(rp, ri, rv, indptr, indices, data, r0, r1))) return rc;
                HIPC(o.alloc(sizeof(double) * (size_t)(rows * (lams ? nch : nt))));
                GramDenseArgs a;
                a.rows = (int)rows;
                a.n2t = (int)nt;
                a.group = group;
                a.cpw = cpw;
                a.degree = degree;
                a.lams_mode = lams ? 1 : 0;
                a.transpose_out = transpose_out ? 1 : 0;
                a.n_chunks = nch;
                a.ebase = indptr[r0];
                a.rptr = rp.as<int64_t>();
                a.ridx = ri.as<int32_t>();
                a.rval = rv.as<double>();
                a.Bt = bt.as<double>();
                a.ldp = nt;
                a.lams = lams ? dl.as<double>() : nullptr;
                a.out = o.as<double>();
                launch(a, dim3((unsigned)cdiv64(rows, rows_per_wg), (unsigned)cdiv64(nch, cpw)),
                       stream);
                HIPC(hipGetLastError());
                if (lams) {
                    if ((rc = finish_lams_block(o, r0, rows, nch, nch_all, j0 == 0, hpart)))
                        return rc;
                } else if ((rc = download_block(o, n1, n2, r0, rows, j0, nt, transpose_out))) {
                    return rc;
                }
                // the block's buffers are reused by the next block
                HIPC(hipStreamSynchronize(stream));
            }
        }
        HIPC(hipStreamSynchronize(stream));
        return SPFM_OK;
    }

    // ------------------------------------------------------------ CSR x CSR
    int csr_csr(int64_t n1, int32_t d, const int64_t* indptr1, const int32_t* indices1,
                const double* data1, int64_t n2, const int64_t* indptr2,
                const int32_t* indices2, const double* data2) {
        int rc = check_kind();
        if (rc) return rc;
        if (n2 < 0 || n2 > INT32_MAX) FAIL(SPFM_ERR_INVALID, "gram: bad n2");
        if ((rc = check_csr("X", n1, d, indptr1, indices1, data1))) return rc;
        if ((rc = check_csr("P", n2, d, indptr2, indices2, data2))) return rc;
        if (n1 == 0 || n2 == 0) return empty_result(n1);
        // P tiles: whole 64-row chunks whose CSR takes <= half the budget (at least one chunk)
        std::vector<int64_t> tiles(1, 0);
        for (int64_t j0 = 0; j0 < n2;) {
            int64_t j = j0, bytes = 8;
            while (j < n2) {
                const int64_t je = std::min(n2, j + kGramChunk);
                const int64_t cb = (je - j) * 8 + (indptr2[je] - indptr2[j]) * 12;
                if (j > j0 && bytes + cb > budget / 2) break;
                bytes += cb;
                j = je;
            }
            tiles.push_back(j);
            j0 = j;
        }
        const int64_t nch_all = cdiv64(n2, kGramChunk);
        CsrLaunch launch = pick_csr(kind, degree);
        DevBuf pp, pi, pv, rp, ri, rv, o, dl;
        std::vector<double> hpart;
        std::vector<int64_t> bounds;
        for (size_t ti = 0; ti + 1 < tiles.size(); ++ti) {
            const int64_t j0 = tiles[ti], nt = tiles[ti + 1] - j0;
            const int nch = (int)cdiv64(nt, kGramChunk);
            int stage = 1;
            for (int c = 0; c < nch; ++c) {
                const int64_t a = j0 + (int64_t)c * kGramChunk;
                const int64_t b = std::min(j0 + nt, a + kGramChunk);
                if (indptr2[b] - indptr2[a] > kGramStageP) stage = 0;
            }
            HIPC(hipStreamSynchronize(stream));
            if ((rc = upload_rows(pp, pi, pv, indptr2, indices2, data2, j0, j0 + nt))) return rc;
            if (lams) SPFM_TRY(eng.upload(dl, lams + j0, (size_t)nt));
            const int64_t tile_bytes = (nt + 1) * 8 + (indptr2[j0 + nt] - indptr2[j0]) * 12;
            const int64_t per_row = lams ? (int64_t)nch * 8 : nt * 8;
            row_blocks(n1, indptr1, per_row, std::max<int64_t>(budget - tile_bytes, 1), bounds);
            for (size_t bi = 0; bi + 1 < bounds.size(); ++bi) {
                const int64_t r0 = bounds[bi], r1 = bounds[bi + 1], rows = r1 - r0;
                if ((rc = upload_rows(rp, ri, rv, indptr1, indices1, data1, r0, r1))) return rc;
                HIPC(o.alloc(sizeof(double) * (size_t)(rows * (lams ? nch : nt))));
                GramCsrArgs a;
                a.rows = (int)rows;
                a.n2t = (int)nt;
                a.degree = degree;
                a.lams_mode = lams ? 1 : 0;
                a.stage_p = stage;
                a.n_chunks = nch;
                a.xbase = indptr1[r0];
                a.xptr = rp.as<int64_t>();
                a.xidx = ri.as<int32_t>();
                a.xval = rv.as<double>();
                a.pbase = indptr2[j0];
                a.pptr = pp.as<int64_t>();
                a.pidx = pi.as<int32_t>();
                a.pval = pv.as<double>();
                a.lams = lams ? dl.as<double>() : nullptr;
                a.out = o.as<double>();
                launch(a, dim3((unsigned)std::min<int64_t>(cdiv64(rows, 4), 8192), (unsigned)nch),
                       stream);
                HIPC(hipGetLastError());
                if (lams) {
                    if ((rc = finish_lams_block(o, r0, rows, nch, nch_all, j0 == 0, hpart)))
                        return rc;
                } else if ((rc = download_block(o, n1, n2, r0, rows, j0, nt, false))) {
                    return rc;
                }
                HIPC(hipStreamSynchronize(stream));
            }
        }
        HIPC(hipStreamSynchronize(stream));
        return SPFM_OK;
    }
};

}  // namespace

extern "C" {

int spfm_gram_csr_dense(spfm_handle h, int kind, int degree, int64_t n1, int32_t d,
                        const int64_t* indptr, const int32_t* indices, const double* data,
                        int64_t n2, const double* B, const double* lams, int transpose_out,
                        int64_t max_block_bytes, double* out) {
    SPFM_GUARD(h);
    GramRun g(*h, kind, degree, lams, max_block_bytes, out);
    return g.csr_dense(n1, d, indptr, indices, data, n2, B, transpose_out);
}

int spfm_gram_csr_csr(spfm_handle h, int kind, int degree, int64_t n1, int32_t d,
                      const int64_t* indptr1, const int32_t* indices1, const double* data1,
                      int64_t n2, const int64_t* indptr2, const int32_t* indices2,
                      const double* data2, const double* lams, int64_t max_block_bytes,
                      double* out) {
    SPFM_GUARD(h);
    GramRun g(*h, kind, degree, lams, max_block_bytes, out);
    return g.csr_csr(n1, d, indptr1, indices1, data1, n2, indptr2, indices2, data2);
}

}  // extern "C"
