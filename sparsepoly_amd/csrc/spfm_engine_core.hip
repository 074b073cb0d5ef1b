// spfm_engine_core.hip -- host engine: data images, parameters, schedule, predict, communicators,
// residency / recovery of the persistent passes, and their part of the C ABI (include/spfm.h).
#include "spfm_engine.hip.h"
#include "spfm_linear.hip.h"   // col_norm_kernel
#include "spfm_predict.hip.h"
#include "spfm_pbcd.hip.h"     // kPbW

using namespace spfm;

static thread_local std::string g_create_error;

// ------------------------------------------------------------------ RCCL (lazy)
// RCCL is loaded with dlopen so that the single-GPU path has no link dependency
// and shares whichever librccl the process already holds (PyTorch ships one).
namespace {
struct ncclUniqueId_ {
    char internal[128];
};
enum { ncclSum_ = 0 };
enum { ncclFloat64_ = 8 };
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(ncclUniqueId_*) = nullptr;
    int (*CommInitRank)(ncclComm_t*, int, ncclUniqueId_, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    const char* (*GetLastError)(ncclComm_t) = nullptr;
    int (*GetVersion)(int*) = nullptr;
    std::string path;  // the file the symbols came from (torch's bundled copy, or ROCm's)
    bool load(std::string& err) {
        if (lib) return true;
        // 1) a copy the process already holds (PyTorch maps its own librccl.so): share it;
        // 2) otherwise load ROCm's, with local scope so that it never interposes on a
        //    copy another library may bring later.
        const char* names[] = {"librccl.so", "librccl.so.1"};
        for (const char* nm : names) {
            lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) {
            const char* fresh[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
            for (const char* nm : fresh) {
                lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
                if (lib) break;
            }
        }
        if (!lib) {
            err = std::string("cannot load librccl: ") + dlerror();
            return false;
        }
        GetUniqueId = (decltype(GetUniqueId))dlsym(lib, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
        AllReduce = (decltype(AllReduce))dlsym(lib, "ncclAllReduce");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        GetLastError = (decltype(GetLastError))dlsym(lib, "ncclGetLastError");
        GetVersion = (decltype(GetVersion))dlsym(lib, "ncclGetVersion");
        Dl_info info;
        if (CommInitRank && dladdr((void*)CommInitRank, &info) && info.dli_fname) path = info.dli_fname;
        if (!GetUniqueId || !CommInitRank || !AllReduce || !CommDestroy) {
            err = "librccl lacks a required symbol";
            return false;
        }
        return true;
    }
};
Rccl g_rccl;
}  // namespace

spfm_engine::~spfm_engine() {
    clear_graphs();
    for (auto& ps : prof)
        for (auto e : ps.ev) (void)hipEventDestroy(e);
    if (comm && g_rccl.CommDestroy) g_rccl.CommDestroy(comm);
    for (size_t r = 0; r < peer_ptr.size(); ++r)
        if (peer_ptr[r] && peer_ptr[r] != peer_own) (void)hipIpcCloseMemHandle(peer_ptr[r]);
    if (peer_own) (void)hipFree(peer_own);
    if (shm.hdr) munmap((void*)shm.hdr, shm.bytes);
    if (h_scalar) (void)hipHostFree(h_scalar);
    if (stream) (void)hipStreamDestroy(stream);
}

// ------------------------------------------------------------------- comm
// sense-reversing barrier over the shm header; bounded (30 s) so that a dead peer
// becomes an error instead of a hang
int spfm_engine::shm_barrier() {
    shm.local_sense ^= 1;
    if (__atomic_add_fetch(&shm.hdr->arrive, 1, __ATOMIC_ACQ_REL) == n_ranks) {
        __atomic_store_n(&shm.hdr->arrive, 0, __ATOMIC_RELAXED);
        __atomic_store_n(&shm.hdr->sense, shm.local_sense, __ATOMIC_RELEASE);
        return SPFM_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&shm.hdr->sense, __ATOMIC_ACQUIRE) != shm.local_sense) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30))
            FAIL(SPFM_ERR_RUNTIME, "shm communicator: peer did not arrive within 30 s");
    }
    return SPFM_OK;
}

int spfm_engine::allreduce_shm(double* buf, size_t count) {
    for (size_t off = 0; off < count; off += ShmComm::kMaxDoubles) {  // long vectors in pieces
        int rc = allreduce_shm_piece(buf + off, std::min(ShmComm::kMaxDoubles, count - off));
        if (rc) return rc;
    }
    return SPFM_OK;
}

int spfm_engine::allreduce_shm_piece(double* buf, size_t count) {
    shm_host.resize(count);
    SPFM_TRY(download(shm_host.data(), buf, count));
    HIPC(hipStreamSynchronize(stream));
    std::memcpy(shm.slots + (size_t)rank * ShmComm::kMaxDoubles, shm_host.data(),
                sizeof(double) * count);
    int rc = shm_barrier();
    if (rc) return rc;
    for (size_t i = 0; i < count; ++i) {  // fixed rank order: identical on every rank
        double a = 0.0;
        for (int r = 0; r < n_ranks; ++r) a += shm.slots[(size_t)r * ShmComm::kMaxDoubles + i];
        shm_host[i] = a;
    }
    rc = shm_barrier();  // nobody overwrites a slot before everyone has read it
    if (rc) return rc;
    SPFM_TRY(upload_to(buf, shm_host.data(), count));
    HIPC(hipStreamSynchronize(stream));
    return SPFM_OK;
}

int spfm_engine::allreduce(double* buf, size_t count) {
    if (shm.hdr) return allreduce_shm(buf, count);
    if (!comm) return SPFM_OK;
    int rc = g_rccl.AllReduce(buf, buf, count, ncclFloat64_, ncclSum_, comm, stream);
    if (rc != 0) {
        err = std::string("ncclAllReduce: ") +
              (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
        return SPFM_ERR_RUNTIME;
    }
    return SPFM_OK;
}

int spfm_engine::ensure_col_norm() {
    if (col_norm_reduced || !dist()) return SPFM_OK;
    int rc = allreduce(col_norm.as<double>(), (size_t)d);
    if (rc) return rc;
    col_norm_reduced = true;
    return SPFM_OK;
}

// --------------------------------------------------------- P <-> Pt images
int spfm_engine::ensure_p() {
    if (p_valid) return SPFM_OK;
    for (int o = 0; o < n_orders; ++o) {
        const size_t off = (size_t)o * k * d;
        hipLaunchKernelGGL(transpose_kernel, dim3(cdiv((int64_t)k * d, 256)), dim3(256), 0,
                           stream, Pt.as<double>() + off, d, k, P.as<double>() + off);
    }
    HIPC(hipGetLastError());
    p_valid = true;
    return SPFM_OK;
}

int spfm_engine::ensure_pt() {
    if (pt_valid) return SPFM_OK;
    HIPC(Pt.alloc(sizeof(double) * (size_t)n_orders * k * d));
    for (int o = 0; o < n_orders; ++o) {
        const size_t off = (size_t)o * k * d;
        hipLaunchKernelGGL(transpose_kernel, dim3(cdiv((int64_t)k * d, 256)), dim3(256), 0,
                           stream, P.as<double>() + off, k, d, Pt.as<double>() + off);
    }
    HIPC(hipGetLastError());
    pt_valid = true;
    return SPFM_OK;
}

// =================================================================== data
// uploads both images; values in CSC order (`data_csc`) or in CSR order (`data_csr`) --
// the other order goes through `perm` (position in the wanted order -> position in the
// given one); conversions to the storage type run on host threads
template <typename T>
int spfm_engine::upload_images(const int64_t* h_cp, const int32_t* h_ci, const int64_t* h_rp,
                  const int32_t* h_ri, const double* data_csc, const double* data_csr,
                  const int64_t* perm, const double* y) {
    std::vector<T> cv((size_t)nnz), rv((size_t)nnz);
    const int T_ = (nnz >= (1 << 20)) ? schedule_threads() : 1;
    {
        std::vector<std::thread> pool;
        auto work = [&](int tid) {
            const int64_t per = (nnz + T_ - 1) / T_;
            const int64_t lo = per * tid, hi = std::min<int64_t>(nnz, lo + per);
            if (data_csc) {
                for (int64_t ii = lo; ii < hi; ++ii) cv[(size_t)ii] = (T)data_csc[ii];
                for (int64_t ii = lo; ii < hi; ++ii) rv[(size_t)ii] = (T)data_csc[perm[ii]];
            } else {
                for (int64_t ii = lo; ii < hi; ++ii) rv[(size_t)ii] = (T)data_csr[ii];
                for (int64_t ii = lo; ii < hi; ++ii) cv[(size_t)ii] = (T)data_csr[perm[ii]];
            }
        };
        for (int t = 1; t < T_; ++t) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    std::vector<T> hy;
    SPFM_TRY(upload(cptr, h_cp, (size_t)d + 1));
    SPFM_TRY(upload(cidx, h_ci, (size_t)nnz));
    SPFM_TRY(upload(cval, cv.data(), (size_t)nnz));
    SPFM_TRY(upload(rptr, h_rp, (size_t)n + 1));
    SPFM_TRY(upload(ridx, h_ri, (size_t)nnz));
    SPFM_TRY(upload(rval, rv.data(), (size_t)nnz));
    HIPC(yy.alloc(sizeof(T) * 2 * (size_t)n));
    SPFM_TRY(upload_targets(y, hy));
    HIPC(col_norm.alloc(sizeof(double) * (size_t)d));
    hipLaunchKernelGGL((col_norm_kernel<T>), dim3(cdiv((int64_t)d * 64, kBlock)),
                       dim3(kBlock), 0, stream, d, cptr.as<int64_t>(), cval.as<T>(),
                       col_norm.as<double>());
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(stream));  // host staging vectors die here
    return SPFM_OK;
}

template <typename T>
int spfm_engine::set_data_t(const int64_t* indptr, const int32_t* indices, const double* data,
               const double* y) {
    std::vector<int64_t> h_rptr, perm;
    std::vector<int32_t> h_ridx;
    csc_to_csr(n, d, indptr, indices, h_rptr, h_ridx, perm);
    return upload_images<T>(indptr, indices, h_rptr.data(), h_ridx.data(), data, nullptr,
                            perm.data(), y);
}

// after the images are on the device: state shared by both ingest forms
int spfm_engine::data_installed(const double* y) {
    if (y) {  // (nullptr: the targets came from another handle, and y_pm1 with them)
        y_pm1 = true;
        for (int64_t i = 0; i < n; ++i)
            if (std::fabs(y[i]) != 1.0) {
                y_pm1 = false;
                break;
            }
    }
    have_data = true;
    configured = false;
    clear_sample_weight();  // they named rows of the old data
    have_sampler = false;  // the positives and the drawn triples named rows of the old data
    sampled = false;
    col_norm_reduced = false;
    invalidate(kInvSchedule | kInvGraphs);
    HIPC(viol_col.alloc(sizeof(double) * (size_t)d));
    HIPC(pred_tmp.alloc(sizeof(double) * (size_t)(n > 0 ? n : 1)));
    HIPC(partial.alloc(sizeof(double) * 1024));
    return SPFM_OK;
}

template <typename T>
int spfm_engine::set_data_csr_device(const int64_t* indptr, const int32_t* indices, const double* data,
                        const double* y) {
    std::vector<T> rv, hy;
    const size_t nz = (size_t)(nnz > 0 ? nnz : 1);
    HIPC(cptr.alloc(sizeof(int64_t) * ((size_t)d + 1)));
    HIPC(cidx.alloc(sizeof(int32_t) * nz));
    HIPC(cval.alloc(sizeof(T) * nz));
    SPFM_TRY(stage_csr_rows(rptr, ridx, rval, rv, indptr, indices, data, 0, n, 1));
    HIPC(yy.alloc(sizeof(T) * 2 * (size_t)(n > 0 ? n : 1)));
    SPFM_TRY(upload_targets(y, hy));
    HIPC(col_norm.alloc(sizeof(double) * (size_t)d));
    HIPC(hipStreamSynchronize(stream));
    int invalid = 0;
    hipError_t e = device_csr_to_csc<T>(n, d, nnz, rptr.as<int64_t>(), ridx.as<int32_t>(),
                                        rval.as<T>(), cptr.as<int64_t>(), cidx.as<int32_t>(),
                                        cval.as<T>(), &invalid, stream);
    if (e != hipSuccess) {  // e.g. no room for the sort's scratch: the host path takes over
        (void)hipGetLastError();
        return kIngestFallback;
    }
    if (invalid)
        FAIL(SPFM_ERR_INVALID,
             "set_data: CSR must have sorted, duplicate-free column indices in [0, d)");
    h_cptr.resize((size_t)d + 1);
    h_cidx.resize((size_t)nnz);
    SPFM_TRY(download(h_cptr.data(), cptr.p, (size_t)d + 1));
    SPFM_TRY(download(h_cidx.data(), cidx.p, (size_t)nnz));
    hipLaunchKernelGGL((col_norm_kernel<T>), dim3(cdiv((int64_t)d * 64, kBlock)), dim3(kBlock), 0,
                       stream, d, cptr.as<int64_t>(), cval.as<T>(), col_norm.as<double>());
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(stream));
    return SPFM_OK;
}

// CSR ingest (replaces get_dataset's X.tocsc(), dataset.py:119-123, too): the CSC image
// is built on the device (above) or by host threads; the CSR image is the input itself
int spfm_engine::set_data_csr(int64_t n_, int32_t d_, const int64_t* indptr, const int32_t* indices,
                 const double* data, const double* y) {
    scache.reset();  // a new image: nothing to share streams with (the allocations detach)
    if (n_ < 0 || d_ <= 0 || !indptr || !y) FAIL(SPFM_ERR_INVALID, "set_data: bad arguments");
    if (n_ >= (int64_t)1 << 31) FAIL(SPFM_ERR_UNSUPPORTED, "n_samples must be < 2^31");
    if (indptr[0] != 0) FAIL(SPFM_ERR_INVALID, "set_data: indptr[0] != 0");
    for (int64_t i = 0; i < n_; ++i)
        if (indptr[i + 1] < indptr[i]) FAIL(SPFM_ERR_INVALID, "set_data: indptr not monotone");
    ingest_device_used = 0;
    if (ingest_device && indptr[n_] < ((int64_t)1 << 31)) {
        if (have_params && d_ != d) have_params = false;
        n = n_;
        d = d_;
        nnz = indptr[n_];
        int rc = SPFM_DISPATCH(dtype, return set_data_csr_device<T>(indptr, indices, data, y));
        if (rc == SPFM_OK) {
            ingest_device_used = 1;
            return data_installed(y);
        }
        if (rc != kIngestFallback) {
            have_data = false;
            return rc;
        }
    }
    std::vector<int64_t> cp, perm;
    std::vector<int32_t> ci;
    if (!csr_to_csc(n_, d_, indptr, indices, cp, ci, perm))
        FAIL(SPFM_ERR_INVALID,
             "set_data: CSR must have sorted, duplicate-free column indices in [0, d)");
    if (have_params && d_ != d) have_params = false;
    n = n_;
    d = d_;
    nnz = indptr[n_];
    h_cptr.swap(cp);
    h_cidx.swap(ci);
    SPFM_TRY(SPFM_DISPATCH(dtype, return upload_images<T>(h_cptr.data(), h_cidx.data(), indptr,
                                                          indices, nullptr, data, perm.data(), y)));
    return data_installed(y);
}

int spfm_engine::set_data(int64_t n_, int32_t d_, const int64_t* indptr, const int32_t* indices,
             const double* data, const double* y) {
    scache.reset();
    if (n_ < 0 || d_ <= 0 || !indptr || !y) FAIL(SPFM_ERR_INVALID, "set_data: bad arguments");
    if (n_ >= (int64_t)1 << 31) FAIL(SPFM_ERR_UNSUPPORTED, "n_samples must be < 2^31");
    if (indptr[0] != 0) FAIL(SPFM_ERR_INVALID, "set_data: indptr[0] != 0");
    for (int j = 0; j < d_; ++j)
        if (indptr[j + 1] < indptr[j]) FAIL(SPFM_ERR_INVALID, "set_data: indptr not monotone");
    const int64_t nz = indptr[d_];
    for (int64_t ii = 0; ii < nz; ++ii)
        if (indices[ii] < 0 || indices[ii] >= n_)
            FAIL(SPFM_ERR_INVALID, "set_data: row index out of range");
    // canonical CSC required: ascending, duplicate-free rows inside each column
    for (int j = 0; j < d_; ++j)
        for (int64_t ii = indptr[j] + 1; ii < indptr[j + 1]; ++ii)
            if (indices[ii] <= indices[ii - 1])
                FAIL(SPFM_ERR_INVALID,
                     "set_data: CSC must have sorted, duplicate-free row indices");
    if (have_params && d_ != d) have_params = false;
    n = n_;
    d = d_;
    nnz = nz;
    h_cptr.assign(indptr, indptr + d + 1);
    h_cidx.assign(indices, indices + nnz);
    SPFM_TRY(SPFM_DISPATCH(dtype, return set_data_t<T>(indptr, indices, data, y)));
    return data_installed(y);
}

// Several handles on ONE matrix (concurrent fits of a regularisation path, one-vs-rest targets):
// `this` refers to src's device image -- CSC, CSR, column norms -- instead of uploading and
// transposing its own (3 GB less per tenant on BASELINE config 2), keeps its own (yhat, y), and
// joins src's stream cache.  The image is freed with its last holder.
static std::mutex g_share_mu;
int spfm_engine::share_data_from(spfm_engine* src, const double* y_) {
    if (!src || src == this) FAIL(SPFM_ERR_INVALID, "share_data: bad source handle");
    if (!src->have_data) FAIL(SPFM_ERR_INVALID, "share_data: the source handle has no data");
    if (src->dtype != dtype || src->device != device)
        FAIL(SPFM_ERR_INVALID, "share_data: both handles need the same device and storage type");
    if (dist() || src->dist())
        FAIL(SPFM_ERR_UNSUPPORTED, "share_data: not with a communicator attached");
    if (have_params && src->d != d) have_params = false;
    n = src->n;
    d = src->d;
    nnz = src->nnz;
    cptr.share(src->cptr);
    cidx.share(src->cidx);
    cval.share(src->cval);
    rptr.share(src->rptr);
    ridx.share(src->ridx);
    rval.share(src->rval);
    col_norm.share(src->col_norm);
    h_cptr = src->h_cptr;
    h_cidx = src->h_cidx;
    ingest_device_used = src->ingest_device_used;
    HIPC(yy.alloc(tsize() * 2 * (size_t)(n > 0 ? n : 1)));
    if (y_ && n > 0) {
        SPFM_TRY(SPFM_DISPATCH(dtype, std::vector<T> hy; SPFM_TRY(upload_targets(y_, hy));
                               return sync()));
    } else if (n > 0) {
        // the source's targets; its stream may still be writing predictions next to them
        HIPC(hipStreamSynchronize(src->stream));
        SPFM_DISPATCH(dtype, hipLaunchKernelGGL((copy_targets_kernel<T>), dim3(cdiv(n, 256)),
                                                dim3(256), 0, stream, n, src->yy.as<T>(),
                                                yy.as<T>()));
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(stream));
        y_pm1 = src->y_pm1;
    }
    {
        std::lock_guard<std::mutex> lk(g_share_mu);
        if (!src->scache) src->scache = std::make_shared<StreamCache>();
        scache = src->scache;
    }
    return data_installed(y_);
}

// ========================================================== row weights
//   The captured graphs of the multi-kernel passes hold kernel arguments and
// the choice of kernel: setting or clearing weights drops them.  An installed schedule stays (a
// valid batch partition is valid on any engine), and so do the entry streams.
void spfm_engine::clear_sample_weight() {
    if (weighted) invalidate(kInvGraphs);
    weighted = false;
    wsum = 0.0;
    wrow.release();
    wcn.release();
}

int spfm_engine::set_sample_weight(const double* weights, int64_t n_) {
    if (!weights) {
        clear_sample_weight();
        return SPFM_OK;
    }
    if (!have_data) FAIL(SPFM_ERR_INVALID, "set_sample_weight: set the data first");
    if (dist())
        FAIL(SPFM_ERR_UNSUPPORTED, "set_sample_weight: not with a communicator attached");
    if (n_ != n) FAIL(SPFM_ERR_INVALID, "set_sample_weight: n differs from the data's rows");
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (!(weights[i] >= 0.0) || !std::isfinite(weights[i]))
            FAIL(SPFM_ERR_INVALID, "set_sample_weight: weight " + std::to_string(i) +
                                       " is negative or not finite");
        sum += weights[i];
    }
    if (!(sum > 0.0)) FAIL(SPFM_ERR_INVALID, "set_sample_weight: all weights are zero");
    if (!std::isfinite(sum)) FAIL(SPFM_ERR_INVALID, "set_sample_weight: the weights' sum is not finite");
    invalidate(kInvGraphs);
    SPFM_TRY(upload(wrow, weights, (size_t)n));
    HIPC(wcn.alloc(sizeof(double) * (size_t)d));
    SPFM_DISPATCH(dtype, hipLaunchKernelGGL((col_norm_w_kernel<T>),
                                            dim3(cdiv((int64_t)d * 64, kBlock)), dim3(kBlock), 0,
                                            stream, d, cptr.as<int64_t>(), cidx.as<int32_t>(),
                                            cval.as<T>(), wrow.as<double>(), wcn.as<double>()));
    HIPC(hipGetLastError());
    SPFM_TRY(sync());  // the caller may reuse its array
    weighted = true;
    wsum = sum;
    return SPFM_OK;
}

// ================================================================= params
int spfm_engine::set_params(int n_orders_, int k_, int32_t d_, const double* P_, const double* w_,
               const double* lams_) {
    if (n_orders_ <= 0 || k_ <= 0 || d_ <= 0 || !P_ || !w_ || !lams_)
        FAIL(SPFM_ERR_INVALID, "set_params: bad arguments");
    if (have_data && d_ != d)
        FAIL(SPFM_ERR_INVALID, "set_params: n_features differs from the data");
    if (!have_data) d = d_;
    for (int s = 0; s < k_; ++s)
        if (std::fabs(lams_[s]) != 1.0) FAIL(SPFM_ERR_INVALID, "Lambdas must be +1 or -1.");
    interaction_release();  // scratch of the interaction passes (sized by the old block)
    rank_release();         // candidate towers of the old parameters
    explain_release();      // slab scratch of the attribution entries
    foldin_release();       // group scratch of the fold-in
    if (n_orders_ != n_orders || k_ != k) {
        configured = false;
        clear_graphs();
    }
    n_orders = n_orders_;
    k = k_;
    h_lams.assign(lams_, lams_ + k);
    SPFM_TRY(upload(P, P_, (size_t)n_orders * k * d));
    SPFM_TRY(upload(w, w_, (size_t)d));
    SPFM_TRY(upload(lams, lams_, (size_t)k));
    HIPC(hipStreamSynchronize(stream));
    p_valid = true;
    pt_valid = false;
    have_params = true;
    return SPFM_OK;
}

int spfm_engine::get_params(double* P_, double* w_) {
    if (!have_params) FAIL(SPFM_ERR_INVALID, "get_params: no parameters set");
    SPFM_TRY(ensure_p());
    if (P_) SPFM_TRY(download(P_, P.p, (size_t)n_orders * k * d));
    if (w_) SPFM_TRY(download(w_, w.p, (size_t)d));
    HIPC(hipStreamSynchronize(stream));
    return SPFM_OK;
}

// ============================================================== configure
int spfm_engine::configure(int solver_, int loss_, int reg_, int top_degree_) {
    if (!have_data || !have_params)
        FAIL(SPFM_ERR_INVALID, "configure: set data and parameters first");
    if (loss_ < 0 || loss_ > 2) FAIL(SPFM_ERR_INVALID, "Loss function not supported.");
    if (reg_ < 0 || reg_ > 5) FAIL(SPFM_ERR_INVALID, "Regularizer not supported.");
    if (solver_ != SPFM_SOLVER_PCD && solver_ != SPFM_SOLVER_PBCD && solver_ != SPFM_SOLVER_PSGD)
        FAIL(SPFM_ERR_INVALID, "Solver is not supported.");
    if (solver_ == SPFM_SOLVER_PSGD) return configure_psgd(loss_, reg_, top_degree_);
    const bool all_subsets = top_degree_ == -1;  // regularizers are called with degree = -1
    if (!all_subsets && top_degree_ < 2)
        FAIL(SPFM_ERR_UNSUPPORTED, "degree must be >= 2 (factorization machine) or -1 (all-subsets)");
    if (top_degree_ > SPFM_MAX_DEGREE)
        FAIL(SPFM_ERR_UNSUPPORTED, "degree > 6 is not supported by the HIP engine");
    if (all_subsets) {
        // sparse_all_subsets.py:33-38: l1 / l21 / omegacs / omegati
        const bool ok_pcd = (reg_ == SPFM_REG_L1 || reg_ == SPFM_REG_OMEGATI);
        const bool ok_pbcd = (reg_ == SPFM_REG_L1 || reg_ == SPFM_REG_L21 || reg_ == SPFM_REG_OMEGACS);
        if ((solver_ == SPFM_SOLVER_PCD && !ok_pcd) || (solver_ == SPFM_SOLVER_PBCD && !ok_pbcd))
            FAIL(SPFM_ERR_INVALID, "this regularizer cannot be used with this solver (all-subsets)");
        if (solver_ == SPFM_SOLVER_PBCD && k > 256)
            FAIL(SPFM_ERR_UNSUPPORTED, "pbcd: n_components > 256 not supported");
    } else if (solver_ == SPFM_SOLVER_PCD) {
        // init_cache_pcd exists only for l1 / squaredl12 / omegati (README.md:28-32)
        if (reg_ != SPFM_REG_L1 && reg_ != SPFM_REG_SQUAREDL12 && reg_ != SPFM_REG_OMEGATI)
            FAIL(SPFM_ERR_INVALID, "this regularizer cannot be used with solver='pcd'");
        if (reg_ == SPFM_REG_SQUAREDL12 && top_degree_ > 2)
            FAIL(SPFM_ERR_INVALID, "SquaredL12 supports only degree=2.");
    } else {
        if (reg_ != SPFM_REG_L1 && reg_ != SPFM_REG_L21 && reg_ != SPFM_REG_SQUAREDL21 &&
            reg_ != SPFM_REG_OMEGACS)
            FAIL(SPFM_ERR_INVALID, "this regularizer cannot be used with solver='pbcd'");
        if (reg_ == SPFM_REG_SQUAREDL21 && top_degree_ != 2)
            FAIL(SPFM_ERR_INVALID, "SquaredL21 supports only degree=2.");
        if (k > 256) FAIL(SPFM_ERR_UNSUPPORTED, "pbcd: n_components > 256 not supported");
    }
    solver = solver_;
    loss = loss_;
    reg = reg_;
    top_degree = top_degree_;
    clear_graphs();
    const size_t ncache = kMaxDegree + 2;
    HIPC(norms.alloc(sizeof(double) * (size_t)d));
    HIPC(cache.alloc(sizeof(double) * ncache * 2));  // pcd: double-buffered per batch
    HIPC(hipMemsetAsync(norms.p, 0, sizeof(double) * (size_t)d, stream));
    HIPC(hipMemsetAsync(cache.p, 0, sizeof(double) * ncache * 2, stream));
    double hd[kMaxDegree + 2] = {0};
    hd[1] = 1.0;  // omegacs.py:46 ; omegati sets it in compute_cache_pcd
    SPFM_TRY(upload(dcache, hd, ncache));
    // pcd keeps the caches of ALL components (one precompute pass per epoch): same
    // footprint as pbcd's (n, (m-1), k) tensor
    const size_t arow = (size_t)(top_degree > 0 ? top_degree - 1 : 1) * k;
    HIPC(A.alloc(tsize() * (size_t)(n > 0 ? n : 1) * arow));
    HIPC(ctl.alloc(sizeof(Ctl)));
    HIPC(hipMemsetAsync(ctl.p, 0, sizeof(Ctl), stream));
    HIPC(comp_order.alloc(sizeof(int32_t) * (size_t)k));
    HIPC(scalar.alloc(sizeof(double) * 8));
    HIPC(pb_ticket.alloc(sizeof(int) * 4));
    if (!h_scalar) HIPC(hipHostMalloc((void**)&h_scalar, sizeof(double) * 8));
    HIPC(hipStreamSynchronize(stream));
    configured = true;
    return alloc_work();
}

int spfm_engine::alloc_work() {
    if (!configured || !have_schedule) return SPFM_OK;
    const size_t per_part = (solver == SPFM_SOLVER_PBCD) ? ((size_t)k + 1) * kPbW : 2;
    const size_t per_delta = (solver == SPFM_SOLVER_PBCD) ? (size_t)k : 1;
    HIPC(part.alloc(sizeof(double) * per_part * (size_t)max_batch_cols));
    HIPC(delta.alloc(sizeof(double) * per_delta * (size_t)max_batch_cols));
    HIPC(pold.alloc(sizeof(double) * per_delta * (size_t)max_batch_cols));
    HIPC(pb_scal.alloc(sizeof(double) * 4 * (size_t)max_batch_cols));
    return SPFM_OK;
}

int spfm_engine::colour_columns(int mode, int64_t rows, const int64_t* cp, const int32_t* ci,
                   bool own, const int32_t* jf, int max_batch) {
    colour_device_used = 0;
    if (mode == SPFM_SCHED_COLORED_RLF) {
        // the device form sits behind the first-fit form's size threshold (below it the host loop
        // is faster than the launches); SPFM_RLF_DEVICE=1 in the environment lifts the threshold
        // so that small problems can exercise the kernels (tests/test_hip_colour_rlf.py)
        const char* env = std::getenv("SPFM_RLF_DEVICE");
        const bool any_size = env && env[0] == '1';
        if (own && colour_device && (any_size || (d >= 4096 && nnz >= (1 << 20))) &&
            nnz < ((int64_t)1 << 31) && rptr.p && cptr.p) {
            int failed = 0;
            const hipError_t e = device_rlf(n, d, nnz, cptr.as<int64_t>(), cidx.as<int32_t>(),
                                            rptr.as<int64_t>(), jf, std::max(1, max_batch), order,
                                            batch_ptr, &failed, stream);
            if (e == hipSuccess && !failed) {
                colour_device_used = 1;
                return SPFM_OK;
            }
            (void)hipGetLastError();
        }
        schedule_rlf(rows, d, cp, ci, jf, std::max(1, max_batch), order, batch_ptr);
        return SPFM_OK;
    }
    // (the test hook "debug_setup_any_size" lifts the size threshold alone)
    if (own && colour_device && (debug_setup_any_size || (d >= 4096 && nnz >= (1 << 20))) &&
        nnz < ((int64_t)1 << 31) && (int64_t)d / std::max(1, max_batch) < 3500 && rptr.p && cptr.p) {
        std::vector<int32_t> col((size_t)d);
        int nc = 0, ovf = 0;
        const hipError_t e = device_first_fit(n, d, nnz, cptr.as<int64_t>(), cidx.as<int32_t>(),
                                              rptr.as<int64_t>(), jf, max_batch, col.data(), &nc,
                                              &ovf, stream);
        if (e == hipSuccess && !ovf && nc > 0) {
            // classes in colour order, their columns in visiting order (stable counting sort)
            std::vector<int32_t> bp((size_t)nc + 1, 0);
            for (int q = 0; q < d; ++q) bp[(size_t)col[(size_t)q] + 1]++;
            for (int c = 0; c < nc; ++c) bp[(size_t)c + 1] += bp[(size_t)c];
            std::vector<int32_t> pos(bp.begin(), bp.end() - 1);
            order.assign((size_t)d, 0);
            for (int q = 0; q < d; ++q) order[(size_t)pos[(size_t)col[(size_t)q]]++] = jf[q];
            batch_ptr = std::move(bp);
            colour_device_used = 1;
            return SPFM_OK;
        }
        (void)hipGetLastError();
    }
    schedule_colored(rows, d, cp, ci, jf, max_batch, order, batch_ptr);
    return SPFM_OK;
}

int spfm_engine::set_schedule(int mode, const int32_t* indices_feature, const int64_t* cf_indptr,
                 const int32_t* cf_indices, int64_t cf_rows, int32_t* order_out,
                 int32_t* n_batches_out) {
    if (!have_data) FAIL(SPFM_ERR_INVALID, "set_schedule: no data");
    if (!indices_feature) FAIL(SPFM_ERR_INVALID, "set_schedule: indices_feature is NULL");
    std::vector<char> seen((size_t)d, 0);
    for (int q = 0; q < d; ++q) {
        const int j = indices_feature[q];
        if (j < 0 || j >= d || seen[(size_t)j])
            FAIL(SPFM_ERR_INVALID, "set_schedule: indices_feature is not a permutation");
        seen[(size_t)j] = 1;
    }
    const int64_t* cp = cf_indptr ? cf_indptr : h_cptr.data();
    const int32_t* ci = cf_indptr ? cf_indices : h_cidx.data();
    const int64_t rows = cf_indptr ? cf_rows : n;
    if (cf_indptr && (!cf_indices || cf_rows <= 0))
        FAIL(SPFM_ERR_INVALID, "set_schedule: bad conflict structure");
    // persistent passes: 64 columns per step; the wide passes (degree-2 pcd, cd_linear) 512
    const bool pers = persistent && (!dist() || peer_ready);
    const bool wide_cfg = wide_on && configured && solver == SPFM_SOLVER_PCD && top_degree == 2;
    const int max_batch =
        pers ? std::min(max_batch_opt, wide_cfg ? 512 : 64) : max_batch_opt;
    if (mode == SPFM_SCHED_EXACT) {
        order.assign(indices_feature, indices_feature + d);
        schedule_exact(rows, d, cp, ci, indices_feature, max_batch, batch_ptr);
    } else if (mode == SPFM_SCHED_COLORED || mode == SPFM_SCHED_COLORED_RLF) {
        colour_columns(mode, rows, cp, ci, !cf_indptr, indices_feature, max_batch);
        if (pers && max_batch > 64 && batch_ptr.size() > 1) {
            // A wide step costs about twice a 64-column step (two fabric hops, 7.0 vs 3.2 us
            // on one GPU): classes of moderate width are cheaper as more, narrower steps.
            // 110 columns per class is where d/64 steps of the 64-column pass equal the
            // classes' count of wide steps; below it, colour again with 64.
            int32_t widest = 0;
            for (size_t b = 0; b + 1 < batch_ptr.size(); ++b)
                widest = std::max(widest, batch_ptr[b + 1] - batch_ptr[b]);
            const double mean_cols = (double)d / (double)(batch_ptr.size() - 1);
            // ... with the 64-column pass's rows in LDS; when the row blocks of 64 workgroups
            // do not fit (float storage: > ~1.1 M rows per GPU; double storage: never) its
            // step costs 5.7 us and the break-even is 80 columns
            // Decided from GLOBAL inputs only (the conflict structure's row count over the
            // ranks, the loss, the options): every rank of a sharded run must
            // cut its sweep into the same steps, or the exchange of the replicated chain
            // mismatches.  Same LDS formula as pcd_pass_prb (degree 2: one cache value).
            int lds_max = 0, ncu = 0;
            HIPC(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock,
                                       device));
            HIPC(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
            const int nr_eff = dist() ? n_ranks : 1;
            const int64_t rows_rank = (rows + nr_eff - 1) / nr_eff;  // largest row shard
            const int Gp = std::max(1, std::min(prb_G, ncu));
            const size_t lds_lr = sizeof(double) * kPrbLdsFixed +
                                  (size_t)((rows_rank + Gp - 1) / Gp) *
                                      (4 + (loss == SPFM_LOSS_SQUARED ? 4 : 5)) + 16;
            // (a non-squared loss keeps its rows in LDS only when all targets are +-1 --
            // the classifiers' case; that rank-local fact is deliberately NOT part of the
            // decision, which must come out the same on every rank without a collective:
            // rank 0 alone may be colouring, bench.py / a cached Schedule)
            const bool rows_fit = dtype == SPFM_F32 && prb_lds && lds_lr <= (size_t)lds_max;
            const double limit = rows_fit ? (double)wide_min_cols : 0.72 * (double)wide_min_cols;
            if (widest > 64 && mean_cols < limit)
                colour_columns(mode, rows, cp, ci, !cf_indptr, indices_feature, 64);
        }
    } else {
        FAIL(SPFM_ERR_INVALID, "set_schedule: unknown mode");
    }
    int rc = install_schedule();
    if (rc) return rc;
    if (order_out) std::memcpy(order_out, order.data(), sizeof(int32_t) * (size_t)d);
    if (n_batches_out) *n_batches_out = (int32_t)batch_ptr.size() - 1;
    return SPFM_OK;
}

// upload order / descriptors / batch boundaries of the schedule in `order`, `batch_ptr`
int spfm_engine::install_schedule() {
    max_batch_cols = 1;
    for (size_t b = 0; b + 1 < batch_ptr.size(); ++b)
        max_batch_cols = std::max(max_batch_cols, batch_ptr[b + 1] - batch_ptr[b]);
    std::vector<ColDesc> hdesc((size_t)d);
    for (int q = 0; q < d; ++q) {
        const int j = order[(size_t)q];
        hdesc[(size_t)q].start = h_cptr[(size_t)j];
        hdesc[(size_t)q].len = (int32_t)(h_cptr[(size_t)j + 1] - h_cptr[(size_t)j]);
        hdesc[(size_t)q].j = j;
    }
    SPFM_TRY(upload(d_order, order.data(), (size_t)d));
    SPFM_TRY(upload(d_desc, hdesc.data(), (size_t)d));
    SPFM_TRY(upload(d_bptr, batch_ptr.data(), batch_ptr.size()));
    HIPC(hipStreamSynchronize(stream));
    {   // FNV-1a over (order, batch_ptr): the schedule's name in a shared stream cache
        uint64_t hsh = 1469598103934665603ull;
        auto mix = [&](const int32_t* v, size_t cnt) {
            for (size_t i = 0; i < cnt; ++i) {
                hsh ^= (uint64_t)(uint32_t)v[i];
                hsh *= 1099511628211ull;
            }
        };
        mix(order.data(), order.size());
        mix(batch_ptr.data(), batch_ptr.size());
        sched_hash = hsh;
    }
    have_schedule = true;
    invalidate(kInvStreams | kInvRelax | kInvPbRelax | kInvGraphs);
    ++sched_version;
    return alloc_work();
}

int spfm_engine::set_schedule_raw(const int32_t* order_in, const int32_t* bptr_in, int32_t nb,
                     const int64_t* cf_indptr, const int32_t* cf_indices, int64_t cf_rows) {
    if (!have_data) FAIL(SPFM_ERR_INVALID, "set_schedule_raw: no data");
    if (!order_in || !bptr_in || nb < 1) FAIL(SPFM_ERR_INVALID, "set_schedule_raw: bad arguments");
    if (bptr_in[0] != 0 || bptr_in[nb] != d)
        FAIL(SPFM_ERR_INVALID, "set_schedule_raw: batch_ptr must run from 0 to n_features");
    std::vector<char> seen((size_t)d, 0);
    for (int q = 0; q < d; ++q) {
        const int j = order_in[q];
        if (j < 0 || j >= d || seen[(size_t)j])
            FAIL(SPFM_ERR_INVALID, "set_schedule_raw: order is not a permutation");
        seen[(size_t)j] = 1;
    }
    const int64_t* cp = cf_indptr ? cf_indptr : h_cptr.data();
    const int32_t* ci = cf_indptr ? cf_indices : h_cidx.data();
    const int64_t rows = cf_indptr ? cf_rows : n;
    if (cf_indptr && (!cf_indices || cf_rows <= 0))
        FAIL(SPFM_ERR_INVALID, "set_schedule_raw: bad conflict structure");
    std::vector<int32_t> stamp((size_t)rows, -1);
    for (int b = 0; b < nb; ++b) {
        if (bptr_in[b + 1] < bptr_in[b])
            FAIL(SPFM_ERR_INVALID, "set_schedule_raw: batch_ptr is not monotone");
        for (int q = bptr_in[b]; q < bptr_in[b + 1]; ++q) {
            const int j = order_in[q];
            for (int64_t ii = cp[j]; ii < cp[j + 1]; ++ii) {
                if (stamp[(size_t)ci[ii]] == b)
                    FAIL(SPFM_ERR_INVALID,
                         "set_schedule_raw: two columns of one batch share a row");
                stamp[(size_t)ci[ii]] = b;
            }
        }
    }
    order.assign(order_in, order_in + d);
    batch_ptr.assign(bptr_in, bptr_in + nb + 1);
    return install_schedule();
}

// ================================================================ predict
template <typename T, int M>
void spfm_engine::launch_anova(int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv,
                  const double* Pt_o, double* out) {
    hipLaunchKernelGGL((anova_predict_kernel<T, M>), dim3(cdiv(rows * 64, kBlock)),
                       dim3(kBlock), 0, stream, rows, k, rp, ri, rv, Pt_o, lams.as<double>(),
                       out);
}

template <typename T>
int spfm_engine::anova_dispatch(int kind, int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv,
                   const double* Pt_o, double* out) {
    if (!SPFM_DISPATCH_KIND(kind, true, launch_anova<T, M>(rows, rp, ri, rv, Pt_o, out)))
        FAIL(SPFM_ERR_UNSUPPORTED, "degree outside 2..6");
    HIPC(hipGetLastError());
    return SPFM_OK;
}

// out (device, f64, length rows) = _get_output on the given CSR image
template <typename T>
int spfm_engine::output_t(int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv, int degree,
             int fit_linear, int add_lower, double* out) {
    if (rows == 0) return SPFM_OK;
    int rc = ensure_p();
    if (rc) return rc;
    pt_valid = false;  // P is the source of truth here
    rc = ensure_pt();
    if (rc) return rc;
    return output_pt_t<T>(rows, rp, ri, rv, degree, fit_linear, add_lower, Pt.as<double>(), out);
}

template <typename T>
int spfm_engine::output_pt_t(int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv,
                             int degree, int fit_linear, int add_lower, const double* Pt_all,
                             double* out) {
    if (rows == 0) return SPFM_OK;
    HIPC(hipMemsetAsync(out, 0, sizeof(double) * (size_t)rows, stream));
    int rc = anova_dispatch<T>(kind_of(degree), rows, rp, ri, rv, Pt_all, out);
    if (rc) return rc;
    if (add_lower) {
        if (n_orders < 2) FAIL(SPFM_ERR_INVALID, "add_lower_deg2 needs P_[1]");
        rc = anova_dispatch<T>(2, rows, rp, ri, rv, Pt_all + (size_t)k * d, out);
        if (rc) return rc;
    }
    if (fit_linear) {
        hipLaunchKernelGGL((linear_predict_kernel<T>), dim3(cdiv(rows, kBlock)), dim3(kBlock),
                           0, stream, rows, rp, ri, rv, w.as<double>(), out);
        HIPC(hipGetLastError());
    }
    return SPFM_OK;
}

// The definition above lives in this unit; spfm_eval_loss (spfm_engine_objective.hip) calls it
// from another one, so the linker needs both storage types emitted here.
template int spfm_engine::output_pt_t<float>(int64_t, const int64_t*, const int32_t*, const float*,
                                             int, int, int, const double*, double*);
template int spfm_engine::output_pt_t<double>(int64_t, const int64_t*, const int32_t*,
                                              const double*, int, int, int, const double*, double*);

template <typename T>
int spfm_engine::init_pred_t(int degree, int fit_linear, int add_lower) {
    int rc = output_t<T>(n, rptr.as<int64_t>(), ridx.as<int32_t>(), rval.as<T>(), degree,
                         fit_linear, add_lower, pred_tmp.as<double>());
    if (rc) return rc;
    if (n > 0) {
        hipLaunchKernelGGL((store_pred_kernel<T>), dim3(cdiv(n, 256)), dim3(256), 0, stream, n,
                           pred_tmp.as<double>(), yy.as<T>());
        HIPC(hipGetLastError());
    }
    return sync();
}

int spfm_engine::init_pred(int degree, int fit_linear, int add_lower) {
    if (!have_data || !have_params) FAIL(SPFM_ERR_INVALID, "init_pred: no data/params");
    have_pred_args = true;
    pa_degree = degree;
    pa_lin = fit_linear;
    pa_lower = add_lower;
    return SPFM_DISPATCH(dtype, return init_pred_t<T>(degree, fit_linear, add_lower));
}

template <typename T>
int spfm_engine::get_y_pred_t(double* out) {
    if (n == 0) return SPFM_OK;
    hipLaunchKernelGGL((load_pred_kernel<T>), dim3(cdiv(n, 256)), dim3(256), 0, stream, n,
                       yy.as<T>(), pred_tmp.as<double>());
    HIPC(hipGetLastError());
    SPFM_TRY(download(out, pred_tmp.p, (size_t)n));
    return sync();
}

template <typename T>
int spfm_engine::loss_sum_t(double* out) {
    const int nb = 512;
    if (weighted)
        hipLaunchKernelGGL((loss_partial_w_kernel<T>), dim3(nb), dim3(kBlock), 0, stream, n,
                           yy.as<typename Vec2<T>::type>(), loss, wrow.as<double>(),
                           partial.as<double>());
    else
        hipLaunchKernelGGL((loss_partial_kernel<T>), dim3(nb), dim3(kBlock), 0, stream, n,
                           yy.as<typename Vec2<T>::type>(), loss, partial.as<double>());
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(kBlock), 0, stream,
                       partial.as<double>(), nb, scalar.as<double>());
    HIPC(hipGetLastError());
    int rc = allreduce(scalar.as<double>(), 1);
    if (rc) return rc;
    SPFM_TRY(download(h_scalar, scalar.p, 1));
    rc = sync();
    if (rc) return rc;
    *out = h_scalar[0];
    return SPFM_OK;
}

template <typename T>
int spfm_engine::predict_csr_t(int64_t rows, const int64_t* indptr, const int32_t* indices,
                  const double* data, int degree, int fit_linear, int add_lower,
                  double* out) {
    if (rows == 0) return SPFM_OK;
    const int64_t nz = indptr[rows];
    for (int64_t ii = 0; ii < nz; ++ii)
        if (indices[ii] < 0 || indices[ii] >= d)
            FAIL(SPFM_ERR_INVALID, "predict: column index out of range");
    std::vector<T> hv;
    DevBuf rp, ri, rv, o;
    SPFM_TRY(stage_csr_rows(rp, ri, rv, hv, indptr, indices, data, 0, rows));
    HIPC(o.alloc(sizeof(double) * (size_t)rows));
    SPFM_TRY(output_t<T>(rows, rp.as<int64_t>(), ri.as<int32_t>(), rv.as<T>(), degree, fit_linear,
                         add_lower, o.as<double>()));
    SPFM_TRY(download(out, o.p, (size_t)rows));
    return sync();
}

// ================================================================== epochs
int spfm_engine::epoch_prologue() {
    if (!have_data || !have_params || !configured)
        FAIL(SPFM_ERR_INVALID, "epoch: data, parameters and configuration are required");
    if (!have_schedule) FAIL(SPFM_ERR_INVALID, "epoch: call spfm_set_schedule first");
    if (weighted && dist())
        FAIL(SPFM_ERR_UNSUPPORTED, "epoch: sample weights with a communicator attached");
    int rc = ensure_col_norm();
    if (rc) return rc;
    HIPC(hipMemsetAsync(viol_col.p, 0, sizeof(double) * (size_t)d, stream));
    return SPFM_OK;
}

int spfm_engine::epoch_epilogue(double* viol) {
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(kBlock), 0, stream,
                       viol_col.as<double>(), d, scalar.as<double>());
    HIPC(hipGetLastError());
    SPFM_TRY(download(h_scalar, scalar.p, 1));
    HIPC(hipStreamSynchronize(stream));
    prof_collect();
    if (viol) *viol = h_scalar[0];
    return SPFM_OK;
}

// ---- residency and recovery of the persistent passes
// All workgroups of a persistent launch must be resident at once (they wait for each other
// inside the kernel).  `fn` with `threads` threads and `lds` bytes of dynamic LDS: do G
// workgroups fit the device (times the ranks that share it in a one-GPU rehearsal)?
bool spfm_engine::resident_ok(const void* fn, int threads, size_t lds, int G) {
    int per_cu = 0;
    auto it = resident_cache.find(fn);
    if (it != resident_cache.end()) {
        per_cu = it->second;
    } else {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) !=
            hipSuccess) {
            (void)hipGetLastError();
            per_cu = 1;  // unknown: the in-kernel time-out stays the safety net
        }
        resident_cache[fn] = per_cu;
    }
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
        return true;
    // host-shm communicator: ranks on one GPU; co_tenants: handles of this process whose
    // persistent passes run side by side (concurrent fits, one stream each)
    const int64_t sharers = (int64_t)(shm.hdr ? n_ranks : 1) * co_tenants;
    const bool mine = (int64_t)per_cu * ncu >= (int64_t)G * sharers;
    if (!dist()) return mine;
    // Several ranks: the verdict must be the same on all of them -- a rank that alone switched to
    // the multi-kernel engine would issue a per-step collective while its peers sit in the
    // in-kernel exchange.  Agreed once per (kernel, grid, sharers): the sum of the ranks' "no".
    char key[96];
    snprintf(key, sizeof key, "%p|%d|%lld|%zu", fn, G, (long long)sharers, lds);
    auto ag = resident_agreed.find(key);
    if (ag != resident_agreed.end()) return ag->second;
    double no = mine ? 0.0 : 1.0;
    bool agreed = mine;
    double* slot = scalar.as<double>() + 7;
    if (scalar.p && upload_to(slot, &no, 1) == SPFM_OK && sync() == SPFM_OK &&
        allreduce(slot, 1) == SPFM_OK && download(&no, slot, 1) == SPFM_OK && sync() == SPFM_OK)
        agreed = no == 0.0;
    resident_agreed[key] = agreed;
    return agreed;
}

int spfm_engine::snapshot_state(const double* params, size_t count, DevBuf& dst) {
    HIPC(dst.alloc(sizeof(double) * count));
    HIPC(hipMemcpyAsync(dst.p, params, sizeof(double) * count, hipMemcpyDeviceToDevice, stream));
    const size_t nc = kMaxDegree + 2;
    HIPC(snapC.alloc(sizeof(double) * nc * 3));
    HIPC(hipMemcpyAsync(snapC.p, cache.p, sizeof(double) * nc * 2, hipMemcpyDeviceToDevice,
                        stream));
    HIPC(hipMemcpyAsync(snapC.as<double>() + nc * 2, dcache.p, sizeof(double) * nc,
                        hipMemcpyDeviceToDevice, stream));
    return SPFM_OK;
}

// did the persistent launches of this epoch time out?  With several ranks the answer is
// agreed on (sum of the flags), so that all of them redo the epoch together.
int spfm_engine::persistent_aborted(bool* out) {
    *out = false;
    if (!prb_abort.p) return SPFM_OK;
    unsigned flag = 0;
    SPFM_TRY(download(&flag, prb_abort.p, 1));
    HIPC(hipStreamSynchronize(stream));
    double any = flag ? 1.0 : 0.0;
    if (dist()) {
        double* slot = scalar.as<double>() + 6;
        SPFM_TRY(upload_to(slot, &any, 1));
        HIPC(hipStreamSynchronize(stream));
        SPFM_TRY(allreduce(slot, 1));
        SPFM_TRY(download(&any, slot, 1));
        HIPC(hipStreamSynchronize(stream));
    }
    if (flag) HIPC(hipMemsetAsync(prb_abort.p, 0, sizeof(unsigned) * 4, stream));
    *out = any != 0.0;
    return SPFM_OK;
}

// after a time-out: parameters and regularizer state back to the epoch's start, y_pred
// recomputed from them, the persistent passes switched off for this handle
int spfm_engine::recover_from_abort(double* params, size_t count, const DevBuf& src, const char* what) {
    pers_failed = true;
    pers_fallbacks += 1;
    pers_reason = std::string(what) +
                  " timed out waiting for its workgroups (not all resident, or a peer GPU "
                  "did not answer)";
    if (getenv("SPFM_VERBOSE")) fprintf(stderr, "spfm: fall-back: %s\n", pers_reason.c_str());
    if (!have_pred_args)
        FAIL(SPFM_ERR_RUNTIME, pers_reason + "; the model is half-updated (no spfm_init_pred "
                                             "call to recompute y_pred from)");
    const size_t nc = kMaxDegree + 2;
    HIPC(hipMemcpyAsync(params, src.p, sizeof(double) * count, hipMemcpyDeviceToDevice, stream));
    HIPC(hipMemcpyAsync(cache.p, snapC.p, sizeof(double) * nc * 2, hipMemcpyDeviceToDevice,
                        stream));
    HIPC(hipMemcpyAsync(dcache.p, snapC.as<double>() + nc * 2, sizeof(double) * nc,
                        hipMemcpyDeviceToDevice, stream));
    clear_graphs();
    return init_pred(pa_degree, pa_lin, pa_lower);
}

// tag 0 = "not yet" in the own exchange slab; all ranks must have passed the previous launch
// before anybody clears (the caller's epochs are collective: one clear per launch, and a
// rank only starts writing to a peer after that peer's clear because the first remote store
// of a launch follows a local sweep that needs ... nothing remote).  To be safe the clear is
// followed by a barrier over the host communicator.
int spfm_engine::peer_clear(size_t off_doubles, size_t n_doubles) {
    if (!peer_ready) return SPFM_OK;
    HIPC(hipMemsetAsync(reinterpret_cast<double*>(peer_own) + off_doubles, 0,
                        sizeof(double) * n_doubles, stream));
    HIPC(hipStreamSynchronize(stream));
    return host_barrier();
}

int spfm_engine::host_barrier() {
    if (shm.hdr) return shm_barrier();
    if (comm) {  // a 1-element all-reduce doubles as the barrier
        int rc = allreduce(scalar.as<double>() + 4, 1);
        if (rc) return rc;
        HIPC(hipStreamSynchronize(stream));
    }
    return SPFM_OK;
}

// ===================================================== the set-up tables, read back (spfm.h)
int spfm_engine::debug_stream_info(int which, int64_t* info) {
    if (!info) FAIL(SPFM_ERR_INVALID, "stream_info: info8 is NULL");
    for (int i = 0; i < 8; ++i) info[i] = 0;
    if (!have_schedule) FAIL(SPFM_ERR_INVALID, "stream_info: no schedule installed");
    switch (which) {
        case SPFM_STREAM_ROWBLOCK:
            if (!prb_ready) FAIL(SPFM_ERR_INVALID, "stream_info: the 64-column stream has not been built");
            info[0] = prb_G, info[1] = n_batches(), info[3] = prb_long, info[5] = nnz;
            info[6] = prb_has_long, info[7] = stream_device_used;
            return SPFM_OK;
        case SPFM_STREAM_ROWBLOCK_RELAXED:
            if (!prb_ready || relax_state != 1)
                FAIL(SPFM_ERR_INVALID, "stream_info: the relaxed runs' stream has not been built");
            info[0] = prb_G, info[1] = (int64_t)r_batch_ptr.size() - 1, info[3] = prb_long;
            info[5] = dbg_r_entries, info[6] = relax_has_long, info[7] = relax_stream_device_used;
            return SPFM_OK;
        case SPFM_STREAM_PBCD:
            if (!pb_stream_ready) FAIL(SPFM_ERR_INVALID, "stream_info: the pbcd stream has not been built");
            info[0] = pb_stream_G, info[1] = n_batches(), info[2] = pb_stream_NG;
            info[4] = pb_stream_balance, info[5] = nnz, info[7] = pb_stream_device_used;
            return SPFM_OK;
        case SPFM_STREAM_WIDE:
            if (!wide_ready) FAIL(SPFM_ERR_INVALID, "stream_info: the wide stream has not been built");
            info[0] = wide_G, info[1] = n_batches(), info[5] = nnz, info[7] = wide_stream_device_used;
            return SPFM_OK;
        default: FAIL(SPFM_ERR_INVALID, "stream_info: unknown kind");
    }
}

int spfm_engine::debug_stream_tables(int which, int32_t* sp, int32_t* src, uint8_t* flags,
                                     uint32_t* lmask, uint8_t* tab, uint8_t* skip,
                                     int32_t* batch_ptr_out) {
    int64_t info[8];
    SPFM_TRY(debug_stream_info(which, info));
    const size_t G = (size_t)info[0], nb = (size_t)info[1], NG = (size_t)info[2];
    const size_t ne = (size_t)info[5];
    const bool relaxed = which == SPFM_STREAM_ROWBLOCK_RELAXED;
    const DevBuf *b_sp, *b_src, *b_flags = nullptr, *b_lmask = nullptr, *b_tab = nullptr;
    size_t nsp;
    if (which == SPFM_STREAM_ROWBLOCK || relaxed) {
        b_sp = relaxed ? &r_sp : &prb_sp;
        b_src = relaxed ? &dbg_r_src : &dbg_prb_src;
        b_lmask = relaxed ? &r_lmask : &prb_lmask;
        nsp = G * nb * 65 + 1;
    } else if (which == SPFM_STREAM_PBCD) {
        b_sp = &pb_sp, b_src = &dbg_pb_src, b_flags = &pb_meta, b_tab = &pb_tab;
        nsp = G * nb * (NG + 1) + 1;
    } else {
        b_sp = &w_wsp, b_src = &dbg_w_src, b_flags = &dbg_w_hz;
        nsp = G * ((size_t)d + nb) + 1;
    }
    if ((lmask && !b_lmask) || (tab && !b_tab) || (flags && !b_flags))
        FAIL(SPFM_ERR_INVALID, "stream_tables: this kind of stream has no such table");
    if ((src && !b_src->p) || (flags && !b_flags->p) ||
        (skip && (!relaxed || dbg_r_skip.size() != (size_t)nnz)))
        FAIL(SPFM_ERR_INVALID,
             "stream_tables: kept only by a handle with debug_setup_any_size = 1 (skip: relaxed runs)");
    HIPC(hipStreamSynchronize(stream));
    if (sp) SPFM_TRY(download(sp, b_sp->p, nsp));
    if (src) SPFM_TRY(download(src, b_src->p, ne));
    if (flags) SPFM_TRY(download(flags, b_flags->p, ne));
    if (lmask) SPFM_TRY(download(lmask, b_lmask->p, G * nb * 2));
    if (tab) SPFM_TRY(download(tab, b_tab->p, G * std::max<size_t>(nb, 1) * 64));
    HIPC(hipStreamSynchronize(stream));
    if (skip && nnz > 0) std::memcpy(skip, dbg_r_skip.data(), (size_t)nnz);
    if (batch_ptr_out) {
        const std::vector<int32_t>& bp = relaxed ? r_batch_ptr : batch_ptr;
        std::memcpy(batch_ptr_out, bp.data(), sizeof(int32_t) * bp.size());
    }
    return SPFM_OK;
}

// ======================================================================= C ABI
extern "C" {

int spfm_create(spfm_handle* out, int device_id, int dtype) {
    if (!out) return SPFM_ERR_INVALID;
    *out = nullptr;
    if (dtype != SPFM_F32 && dtype != SPFM_F64) {
        g_create_error = "dtype must be SPFM_F32 or SPFM_F64";
        return SPFM_ERR_INVALID;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
        return SPFM_ERR_RUNTIME;
    }
    if (device_id < 0 || device_id >= ndev) {
        g_create_error = "device id out of range";
        return SPFM_ERR_INVALID;
    }
    if ((e = hipSetDevice(device_id)) != hipSuccess) {
        g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return SPFM_ERR_RUNTIME;
    }
    spfm_engine* h = new spfm_engine();
    h->device = device_id;
    h->dtype = dtype;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) h->devname = prop.gcnArchName;
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) {
        g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
        delete h;
        return SPFM_ERR_RUNTIME;
    }
    *out = h;
    return SPFM_OK;
}

void spfm_destroy(spfm_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
}

const char* spfm_last_error(spfm_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

#ifndef SPFM_BUILD_TAG
#define SPFM_BUILD_TAG "untagged"
#endif
const char* spfm_build_tag(void) { return SPFM_BUILD_TAG; }

int spfm_device_name(spfm_handle h, char* out, int cap) {
    if (!h || !out || cap <= 0) return SPFM_ERR_INVALID;
    snprintf(out, (size_t)cap, "%s", h->devname.c_str());
    return SPFM_OK;
}

int spfm_set_data_csc(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const double* data, const double* y) {
    SPFM_GUARD(h);
    return h->set_data(n, d, indptr, indices, data, y);
}

int spfm_set_data_csr(spfm_handle h, int64_t n, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const double* data, const double* y) {
    SPFM_GUARD(h);
    return h->set_data_csr(n, d, indptr, indices, data, y);
}

int spfm_share_data(spfm_handle dst, spfm_handle src, const double* y) {
    SPFM_GUARD(dst);
    return dst->share_data_from(src, y);
}

int spfm_set_sample_weight(spfm_handle h, const double* weights, int64_t n) {
    SPFM_GUARD(h);
    return h->set_sample_weight(weights, n);
}

int spfm_get_sample_weight(spfm_handle h, int* set_out, double* sum_out) {
    if (!h) return SPFM_ERR_INVALID;
    if (set_out) *set_out = h->weighted ? 1 : 0;
    if (sum_out) *sum_out = h->weighted ? h->wsum : (double)h->n;
    return SPFM_OK;
}

int spfm_set_params(spfm_handle h, int n_orders, int k, int32_t d, const double* P,
                    const double* w, const double* lams) {
    SPFM_GUARD(h);
    return h->set_params(n_orders, k, d, P, w, lams);
}

int spfm_get_params(spfm_handle h, double* P, double* w) {
    SPFM_GUARD(h);
    return h->get_params(P, w);
}

int spfm_configure(spfm_handle h, int solver, int loss, int regularizer, int top_degree) {
    SPFM_GUARD(h);
    return h->configure(solver, loss, regularizer, top_degree);
}

int spfm_init_pred(spfm_handle h, int degree, int fit_linear, int add_lower_deg2) {
    SPFM_GUARD(h);
    return h->init_pred(degree, fit_linear, add_lower_deg2);
}

int spfm_get_y_pred(spfm_handle h, double* out) {
    SPFM_GUARD(h);
    if (!h->have_data || !out) return SPFM_ERR_INVALID;
    return SPFM_DISPATCH(h->dtype, return h->get_y_pred_t<T>(out));
}

int spfm_loss_sum(spfm_handle h, double* out) {
    SPFM_GUARD(h);
    if (!h->have_data || !h->configured || !out) {
        h->err = "loss_sum: data and configuration required";
        return SPFM_ERR_INVALID;
    }
    return SPFM_DISPATCH(h->dtype, return h->loss_sum_t<T>(out));
}

int spfm_predict_csr(spfm_handle h, int64_t n, const int64_t* indptr, const int32_t* indices,
                     const double* data, int degree, int fit_linear, int add_lower_deg2,
                     double* out) {
    SPFM_GUARD(h);
    if (!h->have_params) {
        h->err = "predict: no parameters set";
        return SPFM_ERR_INVALID;
    }
    if (n < 0 || !indptr || !out) return SPFM_ERR_INVALID;
    return SPFM_DISPATCH(h->dtype, return h->predict_csr_t<T>(n, indptr, indices, data, degree,
                                                              fit_linear, add_lower_deg2, out));
}

int spfm_set_schedule(spfm_handle h, int mode, const int32_t* indices_feature,
                      const int64_t* conflict_indptr, const int32_t* conflict_indices,
                      int64_t conflict_n_rows, int32_t* order_out, int32_t* n_batches_out) {
    SPFM_GUARD(h);
    return h->set_schedule(mode, indices_feature, conflict_indptr, conflict_indices,
                           conflict_n_rows, order_out, n_batches_out);
}

int spfm_set_schedule_raw(spfm_handle h, const int32_t* order, const int32_t* batch_ptr,
                          int32_t n_batches, const int64_t* conflict_indptr,
                          const int32_t* conflict_indices, int64_t conflict_n_rows) {
    SPFM_GUARD(h);
    return h->set_schedule_raw(order, batch_ptr, n_batches, conflict_indptr, conflict_indices,
                               conflict_n_rows);
}

int spfm_get_schedule(spfm_handle h, int32_t* order_out, int32_t* batch_ptr_out,
                      int32_t* n_batches_out) {
    if (!h) return SPFM_ERR_INVALID;
    if (!h->have_schedule) {
        h->err = "get_schedule: no schedule installed";
        return SPFM_ERR_INVALID;
    }
    if (order_out)
        std::memcpy(order_out, h->order.data(), sizeof(int32_t) * h->order.size());
    if (batch_ptr_out)
        std::memcpy(batch_ptr_out, h->batch_ptr.data(), sizeof(int32_t) * h->batch_ptr.size());
    if (n_batches_out) *n_batches_out = (int32_t)h->batch_ptr.size() - 1;
    return SPFM_OK;
}

int spfm_schedule_build(int mode, int64_t n_rows, int32_t d, const int64_t* indptr,
                        const int32_t* indices, const int32_t* indices_feature, int max_batch,
                        int32_t* order_out, int32_t* batch_ptr_out, int32_t* n_batches_out) {
    if (n_rows < 0 || d <= 0 || !indptr || !indices_feature || !order_out || !batch_ptr_out ||
        !n_batches_out)
        return SPFM_ERR_INVALID;
    if (max_batch <= 0) max_batch = 4096;
    std::vector<char> seen((size_t)d, 0);
    for (int q = 0; q < d; ++q) {
        const int j = indices_feature[q];
        if (j < 0 || j >= d || seen[(size_t)j]) return SPFM_ERR_INVALID;
        seen[(size_t)j] = 1;
    }
    std::vector<int32_t> order, bp;
    if (mode == SPFM_SCHED_EXACT) {
        order.assign(indices_feature, indices_feature + d);
        schedule_exact(n_rows, d, indptr, indices, indices_feature, max_batch, bp);
    } else if (mode == SPFM_SCHED_COLORED) {
        schedule_colored(n_rows, d, indptr, indices, indices_feature, max_batch, order, bp);
    } else if (mode == SPFM_SCHED_COLORED_RLF) {
        schedule_rlf(n_rows, d, indptr, indices, indices_feature, max_batch, order, bp);
    } else {
        return SPFM_ERR_INVALID;
    }
    std::memcpy(order_out, order.data(), sizeof(int32_t) * (size_t)d);
    std::memcpy(batch_ptr_out, bp.data(), sizeof(int32_t) * bp.size());
    *n_batches_out = (int32_t)bp.size() - 1;
    return SPFM_OK;
}

int spfm_cd_linear_epoch(spfm_handle h, double alpha, double* viol) {
    SPFM_GUARD(h);
    return h->cd_linear_epoch(alpha, viol);
}

int spfm_pcd_epoch(spfm_handle h, int order_idx, int degree, double beta, double gamma,
                   double eta, const int32_t* indices_component, int n_comp, double* viol) {
    SPFM_GUARD(h);
    return h->pcd_epoch(order_idx, degree, beta, gamma, eta, indices_component, n_comp, viol);
}

int spfm_pbcd_epoch(spfm_handle h, int order_idx, int degree, double beta, double gamma,
                    double eta, double* viol) {
    SPFM_GUARD(h);
    return h->pbcd_epoch(order_idx, degree, beta, gamma, eta, viol);
}

int spfm_host_epoch_begin(spfm_handle h, int order_idx, int degree) {
    SPFM_GUARD(h);
    return h->host_epoch_begin(order_idx, degree);
}
int spfm_host_pass_begin(spfm_handle h, int component) {
    SPFM_GUARD(h);
    return h->host_pass_begin(component);
}
int spfm_host_step_sums(spfm_handle h, int step, double* sums_out) {
    SPFM_GUARD(h);
    return h->host_step(true, step, sums_out, nullptr, nullptr);
}
int spfm_host_step_apply(spfm_handle h, int step, const double* p_new, const double* p_old) {
    SPFM_GUARD(h);
    return h->host_step(false, step, nullptr, p_new, p_old);
}
int spfm_host_epoch_end(spfm_handle h, double* viol) {
    SPFM_GUARD(h);
    return h->host_epoch_end(viol);
}

int spfm_comm_unique_id(char* id128) {
    if (!id128) return SPFM_ERR_INVALID;
    std::string e;
    if (!g_rccl.load(e)) {
        g_create_error = e;
        return SPFM_ERR_RUNTIME;
    }
    ncclUniqueId_ id;
    if (g_rccl.GetUniqueId(&id) != 0) {
        g_create_error = "ncclGetUniqueId failed";
        return SPFM_ERR_RUNTIME;
    }
    std::memcpy(id128, id.internal, 128);
    return SPFM_OK;
}

int spfm_comm_init(spfm_handle h, const char* id128, int n_ranks, int rank) {
    SPFM_GUARD(h);
    if (!id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return SPFM_ERR_INVALID;
    if (!g_rccl.load(h->err)) return SPFM_ERR_RUNTIME;
    ncclUniqueId_ id;
    std::memcpy(id.internal, id128, 128);
    // RCCL checks the HIP runtime's per-thread "last error" at several points of its set-up: an
    // error that an EARLIER, tolerated call of this thread left there (hipFree of a foreign
    // pointer, an occupancy query that was refused, ...) would surface as "unhandled cuda error"
    // from ncclCommInitRank although nothing is wrong now (round 3, gpurun_out/r3_t9.log: the
    // second communicator of a long-lived process, once).  Make sure the stream is idle and the
    // slate is clean before handing over; report what RCCL itself recorded if it still fails.
    (void)hipStreamSynchronize(h->stream);
    const hipError_t stale = h->keep_last_error ? hipSuccess : hipGetLastError();
    int rc = g_rccl.CommInitRank(&h->comm, n_ranks, id, rank);
    if (rc != 0) {
        int ver = 0;
        if (g_rccl.GetVersion) (void)g_rccl.GetVersion(&ver);
        const char* detail = g_rccl.GetLastError ? g_rccl.GetLastError(nullptr) : nullptr;
        h->err = std::string("ncclCommInitRank: ") +
                 (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
        if (detail && *detail) h->err += std::string(" [") + detail + "]";
        h->err += " (librccl " + std::to_string(ver) + " from " + g_rccl.path;
        h->err += std::string("; HIP last error now: ") + hipGetErrorString(hipPeekAtLastError());
        if (stale != hipSuccess)
            h->err += std::string("; cleared before the call: ") + hipGetErrorString(stale);
        h->err += "; set NCCL_DEBUG=INFO for RCCL's own log)";
        h->comm = nullptr;
        return SPFM_ERR_RUNTIME;
    }
    h->n_ranks = n_ranks;
    h->rank = rank;
    h->col_norm_reduced = false;
    h->resident_agreed.clear();
    h->clear_graphs();
    return SPFM_OK;
}

int spfm_comm_init_shm(spfm_handle h, const char* shm_name, int n_ranks, int rank) {
    SPFM_GUARD(h);
    if (!shm_name || n_ranks < 1 || n_ranks > 64 || rank < 0 || rank >= n_ranks)
        return SPFM_ERR_INVALID;
    if (h->comm || h->shm.hdr) {
        h->err = "a communicator is already attached";
        return SPFM_ERR_INVALID;
    }
    using Shm = spfm_engine::ShmComm;
    const size_t bytes = sizeof(Shm::Hdr) + sizeof(double) * Shm::kMaxDoubles * (size_t)n_ranks;
    int fd = shm_open(shm_name, O_RDWR | O_CREAT, 0600);
    if (fd < 0) {
        h->err = std::string("shm_open failed: ") + std::strerror(errno);
        return SPFM_ERR_RUNTIME;
    }
    if (ftruncate(fd, (off_t)bytes) != 0) {  // new segments are zero-filled
        h->err = std::string("ftruncate failed: ") + std::strerror(errno);
        close(fd);
        return SPFM_ERR_RUNTIME;
    }
    void* p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) {
        h->err = std::string("mmap failed: ") + std::strerror(errno);
        return SPFM_ERR_RUNTIME;
    }
    h->shm.hdr = reinterpret_cast<Shm::Hdr*>(p);
    h->shm.slots = reinterpret_cast<double*>(reinterpret_cast<char*>(p) + sizeof(Shm::Hdr));
    h->shm.bytes = bytes;
    h->shm.local_sense = 0;
    h->n_ranks = n_ranks;
    h->rank = rank;
    h->resident_agreed.clear();
    h->col_norm_reduced = false;
    h->clear_graphs();
    return SPFM_OK;
}

int spfm_peer_alloc(spfm_handle h, char* handle64) {
    SPFM_GUARD(h);
    if (!handle64) return SPFM_ERR_INVALID;
    if (!h->peer_own) {
        void* p = nullptr;
        // fine-grained device memory: remote stores become visible to local polling loads
        // without a kernel boundary.  There is NO coarse-grained fall-back: plain hipMalloc
        // memory maps just as well over IPC, but does not promise that visibility, and the first
        // persistent pass would spin into its time-out -- the caller takes the per-step
        // collective instead when this fails (sparsepoly_amd.distributed.connect_peers).
        hipError_t ae = hipExtMallocWithFlags(&p, sizeof(double) * spfm_engine::kPeerDoubles,
                                              hipDeviceMallocFinegrained);
        if (ae != hipSuccess) {
            (void)hipGetLastError();
            h->err = std::string("peer slab: fine-grained device memory is not available (") +
                     hipGetErrorString(ae) + "); use the per-step collective";
            return SPFM_ERR_RUNTIME;
        }
        if (hipMemsetAsync(p, 0, sizeof(double) * spfm_engine::kPeerDoubles, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            (void)hipFree(p);
            h->err = "peer slab memset failed";
            return SPFM_ERR_RUNTIME;
        }
        h->peer_own = p;
    }
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    hipIpcMemHandle_t ih;
    hipError_t e = hipIpcGetMemHandle(&ih, h->peer_own);
    if (e != hipSuccess) {
        h->err = std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e);
        return SPFM_ERR_RUNTIME;
    }
    std::memcpy(handle64, &ih, 64);
    return SPFM_OK;
}

int spfm_peer_connect(spfm_handle h, int n_ranks, int rank, const char* handles) {
    SPFM_GUARD(h);
    if (!handles || n_ranks < 2 || n_ranks > 8 || rank < 0 || rank >= n_ranks)
        return SPFM_ERR_INVALID;
    if (!h->peer_own) {
        h->err = "spfm_peer_connect: call spfm_peer_alloc first";
        return SPFM_ERR_INVALID;
    }
    if (!h->dist() || h->n_ranks != n_ranks || h->rank != rank) {
        h->err = "spfm_peer_connect: attach the communicator (spfm_comm_init[_shm]) with the "
                 "same ranks first";
        return SPFM_ERR_INVALID;
    }
    h->peer_ptr.assign((size_t)n_ranks, nullptr);
    for (int r = 0; r < n_ranks; ++r) {
        if (r == rank) {
            h->peer_ptr[(size_t)r] = h->peer_own;
            continue;
        }
        hipIpcMemHandle_t ih;
        std::memcpy(&ih, handles + (size_t)r * 64, 64);
        void* p = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&p, ih, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            h->err = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e);
            return SPFM_ERR_RUNTIME;
        }
        h->peer_ptr[(size_t)r] = p;
    }
    std::vector<double*> t1((size_t)n_ranks), t2((size_t)n_ranks);
    for (int r = 0; r < n_ranks; ++r) {
        t1[(size_t)r] = reinterpret_cast<double*>(h->peer_ptr[(size_t)r]) + spfm_engine::kPeerPcdOff;
        t2[(size_t)r] = reinterpret_cast<double*>(h->peer_ptr[(size_t)r]) + spfm_engine::kPeerPbOff;
    }
    if (h->upload(h->peer_tab_pcd, t1.data(), (size_t)n_ranks, 8) ||
        h->upload(h->peer_tab_pb, t2.data(), (size_t)n_ranks, 8) || h->sync()) {
        h->err = "peer table upload failed";
        return SPFM_ERR_RUNTIME;
    }
    // handshake: every rank's store into every slab must reach a kernel that is already polling
    // (what the persistent passes assume); all ranks are in this call together
    {
        DevBuf okb;
        int ok = 0;
        h->peer_generation += 1;
        const unsigned long long word = 0x5350464d00000000ull + (unsigned)h->peer_generation;
        const unsigned long long ticks = 100ull * 1000 * 1000 * 10;  // 10 s of the 100 MHz counter
        if (okb.alloc(sizeof(int) * 4) != hipSuccess ||
            hipMemsetAsync(okb.p, 0, sizeof(int) * 4, h->stream) != hipSuccess) {
            h->err = "peer handshake: allocation failed";
            return SPFM_ERR_RUNTIME;
        }
        hipLaunchKernelGGL(peer_probe_kernel, dim3(1), dim3(kWave), 0, h->stream,
                           h->peer_tab_pcd.as<double*>(),
                           spfm_engine::kPeerProbeOff - spfm_engine::kPeerPcdOff, n_ranks, rank,
                           word, ticks, okb.as<int>());
        if (h->download(&ok, okb.p, 1) || h->sync()) {
            h->err = "peer handshake kernel failed";
            return SPFM_ERR_RUNTIME;
        }
        if (!ok) {
            h->err = "peer handshake timed out: a peer's store into this GPU's exchange slab did "
                     "not become visible to a running kernel (use the per-step collective)";
            return SPFM_ERR_RUNTIME;
        }
    }
    h->peer_ready = true;
    // the step cap depends on the engine: set the schedule again
    h->invalidate(spfm_engine::kInvSchedule | spfm_engine::kInvStreams | spfm_engine::kInvGraphs);
    return SPFM_OK;
}

int spfm_profile_enable(spfm_handle h, int on) {
    if (!h) return SPFM_ERR_INVALID;
    h->prof_on = on != 0;
    return SPFM_OK;
}

int spfm_profile_get(spfm_handle h, int which, double* ms, int64_t* launches, int64_t* nnz) {
    if (!h || which < 0 || which > 4) return SPFM_ERR_INVALID;
    if (ms) *ms = h->prof[which].ms;
    if (launches) *launches = h->prof[which].launches;
    if (nnz) *nnz = h->prof[which].nnz;
    return SPFM_OK;
}

int spfm_profile_reset(spfm_handle h) {
    if (!h) return SPFM_ERR_INVALID;
    for (auto& ps : h->prof) {
        ps.ms = 0;
        ps.launches = 0;
        ps.nnz = 0;
        ps.used = 0;
    }
    return SPFM_OK;
}

#include "spfm_options.inc.h"  // spfm_set_option, spfm_get_option and their table

int spfm_debug_prb_stamps(spfm_handle h, long long* out, int cap) {
    SPFM_GUARD(h);
    if ((h->pb_dbg & 8) && out && cap >= 8) {  // diagnostic counters of the persistent pbcd pass
        static unsigned v[16 + 4096];
        if (hipMemcpy(v, h->pb_dbgbuf.p, sizeof v, hipMemcpyDeviceToHost) != hipSuccess)
            return SPFM_ERR_RUNTIME;
        int i = 0;
        for (; i < 16 + 4096 && i < cap; ++i) out[i] = (long long)v[i];
        return i - (i % 16);
    }
    if (h->wide_stamp_on && h->wide_stamps.p && out) {  // wide pcd pass's timers
        const int nv = (int)(h->wide_stamps.bytes / sizeof(long long));
        if (cap < nv) return SPFM_ERR_INVALID;
        if (hipMemcpy(out, h->wide_stamps.p, sizeof(long long) * (size_t)nv,
                      hipMemcpyDeviceToHost) != hipSuccess)
            return SPFM_ERR_RUNTIME;
        return nv;
    }
    if (h->pb_stamp_on && (h->pb_stream_ready || h->pbr_state == 1) && out) {  // persistent pbcd pass's timers
        const int nv = 16 * (h->pbr_state == 1 ? h->pbr_G : h->pb_stream_G);
        if (cap < nv) return SPFM_ERR_INVALID;
        if (hipMemcpy(out, h->pb_stamps.p, sizeof(long long) * (size_t)nv,
                      hipMemcpyDeviceToHost) != hipSuccess)
            return SPFM_ERR_RUNTIME;
        return nv;
    }
    if (!h->prb_ready || !out) return SPFM_ERR_INVALID;
    const int nval = 16 * h->prb_G;
    if (cap < nval) return SPFM_ERR_INVALID;
    if (hipMemcpy(out, h->prb_stamps.p, sizeof(long long) * (size_t)nval, hipMemcpyDeviceToHost) !=
        hipSuccess)
        return SPFM_ERR_RUNTIME;
    return nval;
}

int spfm_debug_hop_latency(spfm_handle h, int partner, int rounds, double* ns_per_hop,
                           int* xcc_ids /* [2] */) {
    SPFM_GUARD(h);
    if (partner < 1 || partner > 255 || rounds < 1 || rounds > (1 << 20) || !ns_per_hop)
        return SPFM_ERR_INVALID;
    DevBuf words, info;
    if (words.alloc(sizeof(unsigned long long) * 32) != hipSuccess ||
        info.alloc(sizeof(int) * 4) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    float best = 1e30f;
    int hinfo[4] = {0, 0, 0, 0};
    for (int rep = 0; rep < 3; ++rep) {  // first repetition warms the code path
        (void)hipMemsetAsync(words.p, 0, sizeof(unsigned long long) * 32, h->stream);
        (void)hipMemsetAsync(info.p, 0, sizeof(int) * 4, h->stream);
        (void)hipEventRecord(e0, h->stream);
        hipLaunchKernelGGL(hop_pingpong_kernel, dim3(partner + 1), dim3(kWave), 0, h->stream,
                           words.as<unsigned long long>(), rounds, partner, info.as<int>());
        (void)hipEventRecord(e1, h->stream);
        if (hipStreamSynchronize(h->stream) != hipSuccess) {
            h->err = "hop_pingpong_kernel failed";
            return SPFM_ERR_RUNTIME;
        }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        (void)hipMemcpy(hinfo, info.p, sizeof(int) * 4, hipMemcpyDeviceToHost);
        if (hinfo[2] != 0) {
            h->err = "hop latency probe: partner workgroup did not respond";
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            return SPFM_ERR_RUNTIME;
        }
        if (rep > 0 && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ns_per_hop = (double)best * 1e6 / (2.0 * rounds);
    if (xcc_ids) {
        xcc_ids[0] = hinfo[0];
        xcc_ids[1] = hinfo[1];
    }
    return SPFM_OK;
}

int spfm_debug_exchange_cost(spfm_handle h, int groups, int ncols, int readers_mod, int rounds,
                             double* ns_per_round) {
    SPFM_GUARD(h);
    if (groups < 1 || groups > 256 || ncols < 1 || ncols > 64 || readers_mod == 0 ||
        rounds < 1 || rounds > (1 << 20) || !ns_per_round)
        return SPFM_ERR_INVALID;
    DevBuf slab, abortw;
    const size_t bytes = sizeof(double) * 2 * (2 * (size_t)groups + 2) * 64 * 2;
    if (slab.alloc(bytes) != hipSuccess || abortw.alloc(16) != hipSuccess) return SPFM_ERR_RUNTIME;
    PrbArgs a{};
    a.G = groups;
    a.slab = slab.as<double>();
    a.abort_flag = abortw.as<unsigned>();
    a.spin_max = 1u << 21;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    (void)hipFuncSetAttribute((const void*)exchange_probe_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->kPrbLds);
    float best = 1e30f;
    unsigned aborted = 0;
    for (int rep = 0; rep < 3; ++rep) {
        (void)hipMemsetAsync(slab.p, 0, bytes, h->stream);
        (void)hipMemsetAsync(abortw.p, 0, 16, h->stream);
        (void)hipEventRecord(e0, h->stream);
        // probe_xcd = x+1: single-XCD variant on XCD x (8x oversized grid, see the kernel)
        hipLaunchKernelGGL(exchange_probe_kernel, dim3(h->probe_xcd ? 8 * groups + 64 : groups),
                           dim3(readers_mod == -12 ? 768 : 512),
                           h->probe_xcd ? (size_t)h->probe_lds : (size_t)h->kPrbLds, h->stream, a,
                           rounds, ncols, readers_mod, h->probe_xcd);
        (void)hipEventRecord(e1, h->stream);
        if (hipStreamSynchronize(h->stream) != hipSuccess) {
            h->err = "exchange_probe_kernel failed";
            return SPFM_ERR_RUNTIME;
        }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        (void)hipMemcpy(&aborted, abortw.p, sizeof(unsigned), hipMemcpyDeviceToHost);
        if (aborted) break;
        if (rep > 0 && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (aborted) {
        h->err = "exchange probe timed out (workgroups not co-resident?)";
        return SPFM_ERR_RUNTIME;
    }
    *ns_per_round = (double)best * 1e6 / rounds;
    return SPFM_OK;
}

int spfm_debug_sweep_sums(spfm_handle h, int groups, int ncols, int nv, int step,
                          const double* vals, double* out) {
    SPFM_GUARD(h);
    if (groups < 1 || groups > 256 || ncols < 1 || ncols > 64 || (nv != 1 && nv != 2) || step < 0 ||
        !vals || !out)
        return SPFM_ERR_INVALID;
    // the slab as the publishing workgroups leave it: [2][groups][64][2] words, parity step & 1
    // filled with the values' bits, the two lowest replaced by the step's tag
    const size_t words = (size_t)2 * groups * 64 * 2;
    const unsigned long long tag = (unsigned long long)(((step >> 1) % 3) + 1);
    std::vector<unsigned long long> host(words, 0ull);
    for (int g = 0; g < groups; ++g)
        for (int q = 0; q < 64; ++q)
            for (int v = 0; v < nv; ++v) {
                unsigned long long u;
                memcpy(&u, vals + ((size_t)g * 64 + q) * nv + v, sizeof u);
                host[(((size_t)(step & 1) * groups + g) * 64 + q) * 2 + v] = (u & ~3ull) | tag;
            }
    DevBuf slab, abortw, dout;
    if (slab.alloc(words * sizeof(double)) != hipSuccess || abortw.alloc(16) != hipSuccess ||
        dout.alloc(sizeof(double) * 64 * 2) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    if (hipMemcpyAsync(slab.p, host.data(), words * sizeof(double), hipMemcpyHostToDevice,
                       h->stream) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    (void)hipMemsetAsync(abortw.p, 0, 16, h->stream);
    (void)hipMemsetAsync(dout.p, 0, sizeof(double) * 64 * 2, h->stream);
    PrbArgs a{};
    a.G = groups;
    a.slab = slab.as<double>();
    a.abort_flag = abortw.as<unsigned>();
    a.spin_max = 1u << 10;  // every tag is there: the sweep cannot spin
    hipLaunchKernelGGL(sweep_probe_kernel, dim3(1), dim3(kPrbThreads), 0, h->stream, a, ncols, nv,
                       step, dout.as<double>());
    if (hipStreamSynchronize(h->stream) != hipSuccess) {
        h->err = "sweep_probe_kernel failed";
        return SPFM_ERR_RUNTIME;
    }
    unsigned aborted = 0;
    (void)hipMemcpy(&aborted, abortw.p, sizeof(unsigned), hipMemcpyDeviceToHost);
    if (aborted) {
        h->err = "sweep probe: a granule did not carry the step's tag";
        return SPFM_ERR_RUNTIME;
    }
    if (hipMemcpy(out, dout.p, sizeof(double) * 64 * nv, hipMemcpyDeviceToHost) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    return SPFM_OK;
}

int spfm_debug_stream_probe(spfm_handle h, int64_t* bytes_out) {
    SPFM_GUARD(h);
    return h->debug_stream_probe(bytes_out);
}

int spfm_debug_write_probe(spfm_handle h, int bytes_per_record, int64_t* bytes_out) {
    SPFM_GUARD(h);
    return h->debug_write_probe(bytes_per_record, bytes_out);
}

int spfm_debug_branch_counts(spfm_handle h, unsigned* out8, int reset) {
    SPFM_GUARD(h);
    if (!out8) return SPFM_ERR_INVALID;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return SPFM_ERR_RUNTIME;
    // one copy of the counters per translation unit that runs chains: add them up
    for (int i = 0; i < BR_COUNT; ++i) out8[i] = 0;
    hipError_t (*const units[])(unsigned*, int) = {
        spfm_branch_counts_pcd,       spfm_branch_counts_prb_f32,   spfm_branch_counts_prb_f64,
        spfm_branch_counts_wide,      spfm_branch_counts_pbcd,      spfm_branch_counts_pbprb_f32,
        spfm_branch_counts_pbprb_f64};
    for (auto unit : units)
        if (unit(out8, reset) != hipSuccess) return SPFM_ERR_RUNTIME;
    return SPFM_OK;
}

int spfm_stream_build(int kind, int64_t n_rows, int32_t d, const int64_t* indptr,
                      const int32_t* indices, const int32_t* order_in, const int32_t* batch_ptr_in,
                      int32_t nb, int groups, int long_thresh, int NG, int balance,
                      const uint8_t* skip, int32_t* sp_out, int32_t* src_out, uint8_t* flags_out,
                      uint32_t* lmask_out, uint8_t* tab_out, int64_t* n_entries) {
    const bool rowblock = kind == SPFM_STREAM_ROWBLOCK || kind == SPFM_STREAM_ROWBLOCK_RELAXED;
    const bool pb = kind == SPFM_STREAM_PBCD, wide = kind == SPFM_STREAM_WIDE;
    if (!(rowblock || pb || wide) || n_rows < 0 || d <= 0 || !indptr || !order_in ||
        !batch_ptr_in || nb < 1 || groups < 1 || !sp_out || !n_entries || (wide && skip))
        return SPFM_ERR_INVALID;
    if (pb && NG != 8 && NG != 16 && NG != 32 && NG != 64) return SPFM_ERR_INVALID;
    // the builders index their arrays with every one of these: check them all first
    if (indptr[0] != 0) return SPFM_ERR_INVALID;
    for (int j = 0; j < d; ++j)
        if (indptr[j + 1] < indptr[j]) return SPFM_ERR_INVALID;
    const int64_t nz = indptr[d];
    if (nz >= ((int64_t)1 << 31) || (nz > 0 && (!indices || !src_out)) ||
        (nz > 0 && !rowblock && !flags_out))
        return SPFM_ERR_INVALID;
    for (int j = 0; j < d; ++j)
        for (int64_t ii = indptr[j]; ii < indptr[j + 1]; ++ii)
            if (indices[ii] < 0 || indices[ii] >= n_rows ||
                (ii > indptr[j] && indices[ii] <= indices[ii - 1]))
                return SPFM_ERR_INVALID;
    std::vector<char> seen((size_t)d, 0);
    for (int q = 0; q < d; ++q) {
        const int j = order_in[q];
        if (j < 0 || j >= d || seen[(size_t)j]) return SPFM_ERR_INVALID;
        seen[(size_t)j] = 1;
    }
    if (batch_ptr_in[0] != 0 || batch_ptr_in[nb] != d) return SPFM_ERR_INVALID;
    for (int b = 0; b < nb; ++b) {
        const int64_t nc = (int64_t)batch_ptr_in[b + 1] - batch_ptr_in[b];
        if (nc < 0 || (!wide && nc > 64)) return SPFM_ERR_INVALID;
    }
    const std::vector<int32_t> order(order_in, order_in + d), bp(batch_ptr_in, batch_ptr_in + nb + 1);
    std::vector<int32_t> sp, src;
    std::vector<uint8_t> flags;
    if (rowblock) {
        std::vector<uint32_t> lmask;
        build_rowblock_stream(n_rows, indptr, indices, order, bp, groups, long_thresh, sp, src, lmask,
                              skip);
        if (lmask_out) std::memcpy(lmask_out, lmask.data(), sizeof(uint32_t) * lmask.size());
    } else if (pb) {
        std::vector<uint8_t> tab;
        build_pb_stream(n_rows, indptr, indices, order, bp, groups, NG, balance != 0, skip, sp, src,
                        flags, tab);
        if (tab_out) std::memcpy(tab_out, tab.data(), tab.size());
    } else {
        std::vector<int32_t> wbase;
        build_wide_stream(n_rows, indptr, indices, order, bp, groups, wbase, sp, src, flags);
    }
    std::memcpy(sp_out, sp.data(), sizeof(int32_t) * sp.size());
    if (!src.empty()) std::memcpy(src_out, src.data(), sizeof(int32_t) * src.size());
    if (!flags.empty()) std::memcpy(flags_out, flags.data(), flags.size());
    *n_entries = (int64_t)src.size();
    return SPFM_OK;
}

int spfm_debug_stream_info(spfm_handle h, int kind, int64_t* info8) {
    SPFM_GUARD(h);
    return h->debug_stream_info(kind, info8);
}

int spfm_debug_stream_tables(spfm_handle h, int kind, int32_t* sp, int32_t* src, uint8_t* flags,
                             uint32_t* lmask, uint8_t* tab, uint8_t* skip,
                             int32_t* batch_ptr_out) {
    SPFM_GUARD(h);
    return h->debug_stream_tables(kind, sp, src, flags, lmask, tab, skip, batch_ptr_out);
}

int spfm_set_use_graph(spfm_handle h, int on) {
    if (!h) return SPFM_ERR_INVALID;
    h->use_graph = on != 0;
    if (!on) h->clear_graphs();
    return SPFM_OK;
}

}  // extern "C"

