// spfm_engine.hip.h -- the host engine behind the C ABI (include/spfm.h): one object per handle.
// The member functions are defined in spfm_engine_*.hip along the engine's seams (core: data,
// parameters, schedule, predict, communicators, recovery, C ABI; pcd: multi-kernel pcd /
// cd_linear and the epoch drivers; prb: persistent 64-column passes, one translation unit per
// storage type; wide: wide persistent passes; pbcd: multi-kernel pbcd; pbprb: persistent pbcd
// pass, one unit per storage type; psgd; gram, objective, interactions (pairs and triples), rank,
// explain, pairs, bank: the read-only feature units).  Every unit owns the extern "C" block of
// its entries.  See DESIGN.md for the execution model.
#pragma once
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <chrono>
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <thread>
#include <vector>

#include "../../include/spfm.h"
#include "spfm_common.hip.h"
#include "spfm_slab_host.h"  // slab_end
#include "spfm_prb.hip.h"    // PrbArgs
#include "spfm_pcdw.hip.h"   // PcdwArgs, PcdwParams
#include "spfm_psgd.hip.h"   // PsgdBatch, PsgdStep (spfm_psgd_host.h)

namespace spfm {
struct IntArgs;  // spfm_interactions.hip.h
void schedule_exact(int64_t, int32_t, const int64_t*, const int32_t*, const int32_t*, int,
                    std::vector<int32_t>&);
void schedule_colored(int64_t, int32_t, const int64_t*, const int32_t*, const int32_t*, int,
                      std::vector<int32_t>&, std::vector<int32_t>&);
void schedule_rlf(int64_t, int32_t, const int64_t*, const int32_t*, const int32_t*, int,
                  std::vector<int32_t>&, std::vector<int32_t>&);
bool csr_to_csc(int64_t, int32_t, const int64_t*, const int32_t*, std::vector<int64_t>&,
                std::vector<int32_t>&, std::vector<int64_t>&);
int schedule_threads();
void csc_to_csr(int64_t, int32_t, const int64_t*, const int32_t*, std::vector<int64_t>&,
                std::vector<int32_t>&, std::vector<int64_t>&);
void build_wide_stream(int64_t, const int64_t*, const int32_t*, const std::vector<int32_t>&,
                       const std::vector<int32_t>&, int, std::vector<int32_t>&,
                       std::vector<int32_t>&, std::vector<int32_t>&, std::vector<uint8_t>&);
void build_pb_stream(int64_t, const int64_t*, const int32_t*, const std::vector<int32_t>&,
                     const std::vector<int32_t>&, int, int, bool, const uint8_t*,
                     std::vector<int32_t>&, std::vector<int32_t>&, std::vector<uint8_t>&,
                     std::vector<uint8_t>&);
void build_rowblock_stream(int64_t, const int64_t*, const int32_t*, const std::vector<int32_t>&,
                           const std::vector<int32_t>&, int, int, std::vector<int32_t>&,
                           std::vector<int32_t>&, std::vector<uint32_t>&, const uint8_t*);
void schedule_relax(int64_t, int32_t, const int64_t*, const int32_t*, const int32_t*, int, int,
                    std::vector<int32_t>&, std::vector<int32_t>&, std::vector<int32_t>&,
                    std::vector<int32_t>&, std::vector<int64_t>&, std::vector<int64_t>&,
                    std::vector<int16_t>&, std::vector<uint8_t>&);
// spfm_ingest.hip: device-side CSR -> CSC (one stable radix sort by column id)
template <typename T>
hipError_t device_csr_to_csc(int64_t, int32_t, int64_t, const int64_t*, const int32_t*, const T*,
                             int64_t*, int32_t*, T*, int*, hipStream_t);
extern template hipError_t device_csr_to_csc<float>(int64_t, int32_t, int64_t, const int64_t*,
                                                    const int32_t*, const float*, int64_t*,
                                                    int32_t*, float*, int*, hipStream_t);
extern template hipError_t device_csr_to_csc<double>(int64_t, int32_t, int64_t, const int64_t*,
                                                     const int32_t*, const double*, int64_t*,
                                                     int32_t*, double*, int*, hipStream_t);
// spfm_ingest.hip: the row-block entry stream on the device (same result as build_rowblock_stream)
hipError_t device_rowblock_stream(int64_t, int32_t, int64_t, int, int, int, const int32_t*,
                                  const int32_t*, const int64_t*, const int32_t*, const uint8_t*,
                                  int32_t*, int32_t*, uint32_t*, int*, int64_t*, hipStream_t);
// spfm_ingest.hip: the pbcd and wide entry streams on the device (same tables as build_pb_stream /
// build_wide_stream)
hipError_t device_pb_stream(int64_t, int32_t, int64_t, int, int, int, int, const int32_t*,
                            const int32_t*, const int64_t*, const int32_t*, const int64_t*,
                            const int32_t*, int32_t*, int32_t*, uint8_t*, uint8_t*, hipStream_t);
hipError_t device_wide_stream(int64_t, int32_t, int64_t, int, int, const int32_t*, const int32_t*,
                              const int64_t*, const int32_t*, const int64_t*, const int32_t*,
                              int32_t*, int32_t*, uint8_t*, hipStream_t);
// spfm_colour.hip: the first-fit colouring on the device (same result as schedule_colored)
hipError_t device_first_fit(int64_t, int32_t, int64_t, const int64_t*, const int32_t*, const int64_t*,
                            const int32_t*, int, int32_t*, int*, int*, hipStream_t);
// ... and the RLF colouring (same result as schedule_rlf)
hipError_t device_rlf(int64_t, int32_t, int64_t, const int64_t*, const int32_t*, const int64_t*,
                      const int32_t*, int, std::vector<int32_t>&, std::vector<int32_t>&, int*,
                      hipStream_t);
}  // namespace spfm

using namespace spfm;
struct IntPass;  // spfm_engine_interactions.hip: what a pass over pairs or triples is

typedef struct ncclComm* ncclComm_t;

// --------------------------------------------------------------------- buffers
// A device allocation.  Several DevBufs (of different handles) may refer to ONE allocation
// (`share`: the matrix image and the entry streams of co-tenant fits, spfm_share_data); the
// memory is freed with its last holder.  `alloc` on a shared buffer detaches first, so a handle
// can never write into -- or resize under -- memory that another handle reads.
struct DevBuf {
    struct Block {
        void* p;
        std::atomic<int> refs;
    };
    Block* blk = nullptr;
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (blk && blk->refs.fetch_sub(1) == 1) {
            (void)hipFree(blk->p);
            delete blk;
        }
        blk = nullptr;
        p = nullptr;
        bytes = 0;
    }
    bool shared() const { return blk && blk->refs.load() > 1; }
    hipError_t alloc(size_t b) {
        if (b <= bytes && p && !shared()) return hipSuccess;
        release();
        if (b == 0) b = 16;
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, b);
        if (e != hipSuccess) return e;
        blk = new Block{q, {1}};
        p = q;
        bytes = b;
        return e;
    }
    void share(const DevBuf& o) {  // refer to o's allocation (read-only by convention)
        if (o.blk == blk) return;
        release();
        if (!o.blk) return;
        o.blk->refs.fetch_add(1);
        blk = o.blk;
        p = o.p;
        bytes = o.bytes;
    }
    template <typename U>
    U* as() const {
        return reinterpret_cast<U*>(p);
    }
};

#define HIPC(expr)                                                                       \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            err = std::string(#expr) + ": " + hipGetErrorString(_e);                     \
            return SPFM_ERR_RUNTIME;                                                     \
        }                                                                                \
    } while (0)

#define FAIL(code, msg) \
    do {                \
        err = (msg);    \
        return (code);  \
    } while (0)

// propagate the status of an engine call
#define SPFM_TRY(call)       \
    do {                     \
        int _rc = (call);    \
        if (_rc) return _rc; \
    } while (0)

// first lines of every extern "C" entry that touches the device
#define SPFM_GUARD(h)                              \
    if (!(h)) return SPFM_ERR_INVALID;             \
    if (hipSetDevice((h)->device) != hipSuccess) { \
        (h)->err = "hipSetDevice failed";          \
        return SPFM_ERR_RUNTIME;                   \
    }

// The one place that maps a handle's storage type to a C++ type: runs the statement with
// T = float or double, e.g. SPFM_DISPATCH(dtype, return init_pred_t<T>(degree, lin, lower)).
#define SPFM_DISPATCH(dt, ...)                                    \
    ((dt) == SPFM_F32 ? [&] { using T = float; __VA_ARGS__; }()   \
                      : [&] { using T = double; __VA_ARGS__; }())

// The one place that maps a component count to the lanes of a group in the psgd unit's kernels:
// runs the statement with L = 16, 32 or 64 (more than 64 components: chunks of 64), e.g.
// SPFM_DISPATCH(dtype, return SPFM_DISPATCH_L(k, return psgd_epoch_tl<T, L>(st))).
#define SPFM_DISPATCH_L(k_, ...)                                      \
    ((k_) <= 16   ? [&] { constexpr int L = 16; __VA_ARGS__; }()      \
     : (k_) <= 32 ? [&] { constexpr int L = 32; __VA_ARGS__; }()      \
                  : [&] { constexpr int L = 64; __VA_ARGS__; }())

// The one place that maps a run-time model kind -- a degree 2..6, or 0 (all-subsets) where AS
// says the caller has that form -- to a compile-time M: runs the statement with M, e.g.
// SPFM_DISPATCH_KIND(kind_of(degree), true, launch_anova<T, M>(rows, ...)).  False, and nothing
// run, for any other kind: the caller reports it in its own words.
template <bool AS, typename F>
static inline bool dispatch_kind(int kind, F&& f) {
    switch (kind) {
        case 0:
            if constexpr (AS) return f(std::integral_constant<int, 0>{}), true;
            return false;
        case 2: return f(std::integral_constant<int, 2>{}), true;
        case 3: return f(std::integral_constant<int, 3>{}), true;
        case 4: return f(std::integral_constant<int, 4>{}), true;
        case 5: return f(std::integral_constant<int, 5>{}), true;
        case 6: return f(std::integral_constant<int, 6>{}), true;
        default: return false;
    }
}
#define SPFM_DISPATCH_KIND(kind, AS, ...)               \
    dispatch_kind<AS>((kind), [&](auto m_) {            \
        constexpr int M = decltype(m_)::value;          \
        __VA_ARGS__;                                    \
    })

static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }
static inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// Lists of one slab of a streaming top-K selection (spfm_select.hip.h): the sorted per-strip
// lists (values, ids) and the merged ones
struct SelBufs {
    DevBuf lv, li, ov, oi;
    hipError_t alloc(int n_strips, int64_t slab, int K) {
        const size_t on = (size_t)slab * K, ln = (size_t)n_strips * on;
        hipError_t e = lv.alloc(sizeof(double) * ln);
        if (e == hipSuccess) e = li.alloc(sizeof(int32_t) * ln);
        if (e == hipSuccess) e = ov.alloc(sizeof(double) * on);
        if (e == hipSuccess) e = oi.alloc(sizeof(int32_t) * on);
        return e;
    }
    // the merged slots of nrow rows before a slab: id -1, every value byte `vbyte`
    hipError_t clear(int64_t nrow, int K, int vbyte, hipStream_t s) {
        hipError_t e = hipMemsetAsync(ov.p, vbyte, sizeof(double) * (size_t)nrow * K, s);
        if (e == hipSuccess) e = hipMemsetAsync(oi.p, 0xFF, sizeof(int32_t) * (size_t)nrow * K, s);
        return e;
    }
    size_t bytes() const { return lv.bytes + li.bytes + ov.bytes + oi.bytes; }
    void release() {
        for (DevBuf* b : {&lv, &li, &ov, &oi}) b->release();
    }
};

// device time of the kernels of one call (not its copies): one event pair, read after each
// slab's sync (spfm_rank_info, spfm_explain_info)
struct DeviceTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms = 0.0;
    DeviceTimer() {
        if (hipEventCreate(&e0) != hipSuccess) e0 = nullptr;
        if (hipEventCreate(&e1) != hipSuccess) e1 = nullptr;
    }
    ~DeviceTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void begin(hipStream_t s) {
        if (e0 && e1) (void)hipEventRecord(e0, s);
    }
    void end(hipStream_t s) {
        if (e0 && e1) (void)hipEventRecord(e1, s);
    }
    void collect() {  // after a sync
        float t = 0.f;
        if (e0 && e1 && hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms += t;
    }
};

// Entry streams of the persistent passes, shared by the handles that share one data image
// (spfm_share_data): whoever needs a stream first builds it (under the lock: co-tenant fits of
// one schedule do not build it twice), the others refer to the same device buffers.  The two
// most recent streams of each kind are kept (shuffle=True makes a new one per iteration).
struct StreamCache {
    std::mutex mu;
    struct Prb {
        std::string key;
        DevBuf sp, erow, eval, lmask;
        int has_long = 0;
    };
    struct Pb {
        std::string key;
        DevBuf sp, erow, eval, meta, tab;
    };
    std::vector<std::unique_ptr<Prb>> prb;
    std::vector<std::unique_ptr<Pb>> pb;
    static constexpr size_t kKeep = 2;
};

struct ProfSlot {
    std::vector<hipEvent_t> ev;  // pairs
    size_t used = 0;
    double ms = 0.0;
    int64_t launches = 0, nnz = 0;
};

struct spfm_engine {
    int device = 0, dtype = SPFM_F32;
    hipStream_t stream = nullptr;
    std::string err;
    std::string devname;

    // data
    int64_t n = 0, nnz = 0;
    int d = 0;
    bool have_data = false;
    DevBuf cptr, cidx, cval, rptr, ridx, rval, yy, A, col_norm;
    std::vector<int64_t> h_cptr;
    std::vector<int32_t> h_cidx;
    bool col_norm_reduced = false;
    // several handles on one matrix (concurrent fits, spfm_share_data): the image buffers above
    // are then shared allocations, and so are the entry streams the handles build
    std::shared_ptr<StreamCache> scache;
    uint64_t sched_hash = 0;  // of (order, batch_ptr): names a schedule in `scache`
    int share_data_from(spfm_engine* src, const double* y);

    // Row weights: per handle like `yy` -- w_i as f64[n] and the weighted
    // column norms cn_j = sum_i w_i x_ij^2 as f64[d] (col_norm belongs to the shared image).
    // While set, the epochs run on the multi-kernel engine and the psgd kernels (the *_usable
    // predicates below); new data clears them (data_installed).
    DevBuf wrow, wcn;
    bool weighted = false;
    double wsum = 0.0;
    int set_sample_weight(const double* weights, int64_t n_);
    void clear_sample_weight();
    int refuse_weighted(const char* what) {
        if (weighted)
            FAIL(SPFM_ERR_UNSUPPORTED, std::string(what) + ": not on a handle with sample weights "
                                                           "(spfm_set_sample_weight)");
        return SPFM_OK;
    }

    // params
    int n_orders = 0, k = 0;
    bool have_params = false;
    DevBuf P, Pt, w, lams;
    bool p_valid = true, pt_valid = false;  // which of P (k,d) / Pt (d,k) is current
    std::vector<double> h_lams;

    // config
    int solver = -1, loss = 0, reg = 0, top_degree = 0;
    bool configured = false;
    DevBuf norms, cache, dcache;

    // schedule
    std::vector<int32_t> order, batch_ptr;
    DevBuf d_order, d_desc;
    int max_batch_cols = 0;
    bool have_schedule = false;
    int64_t sched_version = 0;

    // work
    DevBuf part, delta, pold, viol_col, scalar, ctl, comp_order, pred_tmp, partial, pb_scal,
        pb_ticket;
    bool pbcd_fuse = true;  // prep + chain in one launch (ticket hand-off)
    double* h_scalar = nullptr;  // pinned

    // psgd (minibatch solver): gradient accumulators, sample order, Michelot state
    DevBuf sg_gradP, sg_gradw, sg_samples, sg_part, sg_cond, sg_thr, sg_theta, sg_done,
        sg_norms, sg_conv, sg_sched, sg_idx, sg_snapP, sg_snapw, sg_snapc;
    bool psgd_force_eager = false;
    int psgd_graph_sweeps = 4;
    bool psgd_warm = false;  // sg_cond holds thresholds of a previous minibatch
    int psgd_redone = 0;  // epochs that fell back from graph replay to eager launches
    std::vector<PsgdBatch> h_sched;

    // graphs
    bool use_graph = true;
    bool fuse_chain = true;  // fused chain+sync kernel for batches of <= 64 columns
    int max_batch_opt = 4096;

    // Recovery from a persistent pass that could not run to its end (a workgroup not resident,
    // a peer that never answers): the epoch is all-or-nothing like the reference's
    // (pcd.py:71-137).  Parameters and regularizer state are snapshot before the launches; after
    // a time-out they are restored, y_pred is recomputed from them (the arguments of the last
    // spfm_init_pred) and the epoch is redone on the multi-kernel engine, which this handle then
    // keeps using.  `pers_fallbacks` counts the events (option "persistent_fallbacks").
    bool pers_failed = false;
    int pers_fallbacks = 0;
    std::string pers_reason;
    int spin_max = 1 << 21;  // polls of one in-kernel wait before the pass gives up
    int debug_drop = 0;            // test hook: the next N persistent launches lack a workgroup
    bool keep_last_error = false;  // test hook (spfm_comm_init)
    bool have_pred_args = false;
    int pa_degree = 0, pa_lin = 0, pa_lower = 0;
    DevBuf snapP, snapW, snapC;
    std::map<const void*, int> resident_cache;  // kernel -> workgroups that can be resident
    std::map<std::string, bool> resident_agreed;  // several ranks: the verdict all of them took

    // persistent row-block pass (single GPU, pcd): one launch per component pass
    bool persistent = true;
    int prb_G = 64;
    bool prb_lds = true;  // keep the row block (A, residual) in LDS when it fits (f32, squared)
    int prb_lds_active = 0;  // what the last pcd pass actually used (0 / 1 residual / 2 sign)
    bool y_pm1 = false;      // every target is +1 or -1
    bool prb_ready = false;
    int prb_has_long = 0;
    int prb_long = kPrbLong;  // entries per (workgroup, step, slot) above which a slot is "long"
    DevBuf prb_sp, prb_erow, prb_eval, prb_slab, prb_abort, prow_old, d_bptr, prb_stamps,
        prb_viol, prb_cn, prb_lmask, prb_rec;
    bool prb_pack = true;    // degree-3 passes with rows in global memory: packed row records
    int prb_pack_active = 0;  // what the last pcd pass used
    bool prb_stamp_on = false;
    int wide_min_cols = 110;     // mean class width below which 64-column steps are used instead
    bool wide_stamp_on = false;  // pcdw_stamps: phase timers of the wide pcd pass (float storage)
    DevBuf wide_stamps;
    DevBuf w_rec;  // packed row records of the wide pcd pass (rows in global memory)
    static constexpr size_t kPrbLds = 84 * 1024;  // > half of the CU's 160 KiB: 1 WG per CU
    // relaxed runs: for a schedule of tiny steps (the reference order: 2.6 columns
    // per step) the degree-2 pcd pass merges consecutive steps into runs of ~20 columns whose few
    // shared rows the chains replay; its own boundaries, entry stream and conflict tables
    bool relax_on = true;
    int relax_state = 0;  // 0 not tried for this schedule, 1 in use, -1 not worth it
    std::vector<int32_t> r_batch_ptr;
    int relax_has_long = 0;
    DevBuf r_bptr, r_sp, r_erow, r_eval, r_lmask, r_cfptr, r_cf, r_clist, r_cslab;
    // wide persistent passes (spfm_pcdw.hip.h): steps of up to 512 columns, degree-2 pcd and
    // cd_linear; chosen when the schedule has a step of more than 64 columns
    bool wide_on = true;
    int pcdw_G = 0;  // workgroups of the wide pass; 0 = chosen from the rows (wide_groups)
    bool wide_ready = false;
    int wide_G = 0, wide_tot = 0;
    int wide_lr_active = 0;  // what the last wide pass used: 0 global rows, 1 all rows in LDS, 2 the first rows of a block in LDS
    int wide_lds_cap = -1;   // option "wide_lds_rows" (see wide_launch)
    bool wide_ep = true;     // option "wide_ep": rows (also) in global memory -> entry-parallel form
    int wide_ep_active = 0;  // what the last wide pass used
    bool wide_rec8 = true;   // option "wide_rec8": squared loss, float: 8-byte (A, residual) row records
    DevBuf w_wbase, w_wsp, w_erow, w_eval, w_slabA, w_slabB;
    // persistent pbcd pass (spfm_pbprb.hip.h): its own workgroup count, hence its own entry
    // stream when that differs from the pcd / cd_linear pass's
    bool pb_persistent = true;
    int pbprb_G = 256;
    int probe_xcd = 0, probe_lds = 60 * 1024;  // diagnostics (spfm_debug_exchange_cost)
    bool pb_stream_ready = false;
    int pb_stream_G = 0, pb_stream_NG = 0;
    DevBuf pb_tab;            // its (workgroup, step) -> slot groups map (gtab)
    // relaxed runs of the persistent pbcd pass (pbcd_prb_kernel CR): merged step boundaries,
    // their entry stream, the conflict tables
    int pbr_state = 0;        // 0 not tried for this schedule, 1 in use, -1 not worth it
    int pbr_G = 0, pb_relax_active = 0;
    std::vector<int32_t> pbr_batch_ptr;
    DevBuf pbr_bptr, pbr_sp, pbr_erow, pbr_eval, pbr_meta, pbr_tab, pbr_cfptr, pbr_cf, pbr_clist,
        pbr_slabR;
    bool pb_balance = true;   // balanced slot groups (0: the fixed map slot q -> group q % NG)
    DevBuf pb_sp, pb_erow, pb_eval, pb_meta, pb_slabA, pb_slabB, pb_slabC, pb_stamps, pb_rec;
    bool pb_stamp_on = false;
    int pbprb_active = 0;  // what the last pbcd epoch used
    int pb_dbg = 0;
    DevBuf pb_dbgbuf;
    std::map<std::string, hipGraphExec_t> graphs;

    // comm
    ncclComm_t comm = nullptr;
    // Host shared-memory communicator (spfm_comm_init_shm): the same sharded protocol with
    // the all-reduce done through a POSIX shm segment, for ranks that share ONE GPU (RCCL
    // refuses two ranks per device) -- exercises the multi-GPU path on a single-GPU box.
    struct ShmComm {
        static constexpr size_t kMaxDoubles = 1 << 16;
        struct Hdr {
            volatile int arrive;
            volatile int sense;
            int pad[14];
        };
        Hdr* hdr = nullptr;
        double* slots = nullptr;  // [n_ranks][kMaxDoubles]
        size_t bytes = 0;
        int local_sense = 0;
    } shm;
    std::vector<double> shm_host;
    bool dist() const { return comm != nullptr || shm.hdr != nullptr; }
    int n_ranks = 1, rank = 0;
    // In-kernel cross-GPU exchange of the persistent passes (spfm_peer_alloc / _connect): one
    // exchange slab per GPU, mapped into every rank (hipIpc); the kernels write their GPU's
    // per-step totals into every GPU's slab and poll their own -- no per-step collective.
    // Layout (doubles): [0, 16K) pcd / cd_linear [2][n_ranks][64][2]; [16K, ...) pbcd
    // [2][64][n_ranks][64].
    static constexpr size_t kPeerPcdOff = 0, kPeerPbOff = 16 * 1024;
    static constexpr size_t kPeerProbeOff = kPeerPbOff + (size_t)2 * 64 * 8 * 64;  // [8] handshake
    static constexpr size_t kPeerDoubles = kPeerProbeOff + 64;
    int peer_generation = 0;  // connects so far (the handshake word differs per connect)
    void* peer_own = nullptr;
    std::vector<void*> peer_ptr;     // [n_ranks] mapped bases ([rank] = own)
    DevBuf peer_tab_pcd, peer_tab_pb;  // device tables of the per-kernel region pointers
    bool peer_ready = false;

    // profile
    bool prof_on = false;
    ProfSlot prof[5];

    ~spfm_engine();

    void clear_graphs() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
    }

    // What a change of an option, the schedule or the engine makes stale (the masks of
    // spfm_options.inc.h).  The only place that resets the readiness and relax flags; the
    // builders set them again when they next run.
    enum : unsigned {
        kInvPrbStream = 1,    // entry stream of the 64-column pass
        kInvPbStream = 2,     // entry stream of the persistent pbcd pass
        kInvWideStream = 4,   // entry stream of the wide pass
        kInvRelax = 8,        // relaxed runs of the pcd pass
        kInvPbRelax = 16,     // relaxed runs of the pbcd pass
        kInvSchedule = 32,    // the schedule has to be set again
        kInvGraphs = 64,      // captured graphs
        kInvStreams = kInvPrbStream | kInvPbStream | kInvWideStream,
    };
    void invalidate(unsigned mask) {
        if (mask & kInvPrbStream) prb_ready = false;
        if (mask & kInvPbStream) pb_stream_ready = false;
        if (mask & kInvWideStream) wide_ready = false;
        if (mask & kInvRelax) relax_state = 0;
        if (mask & kInvPbRelax) pbr_state = 0;
        if (mask & kInvSchedule) have_schedule = false;
        if (mask & kInvGraphs) clear_graphs();
    }

    RegState regstate() {
        RegState rs;
        rs.norms = norms.as<double>();
        rs.cache = cache.as<double>();
        rs.dcache = dcache.as<double>();
        return rs;
    }

    size_t tsize() const { return dtype == SPFM_F32 ? 4 : 8; }

    int sync() {
        HIPC(hipStreamSynchronize(stream));
        return SPFM_OK;
    }

    // ---------------------------------------------------------------- typed copies
    // `count` elements of the host pointer's type, asynchronous on `stream`.  Nothing is issued
    // for a count of 0 and nothing waits: host memory stays alive until the caller's next sync().
    template <typename U>
    int upload_to(void* dst, const U* src, size_t count) {  // into device memory that exists
        if (count) HIPC(hipMemcpyAsync(dst, src, sizeof(U) * count, hipMemcpyHostToDevice, stream));
        return SPFM_OK;
    }
    // (re)allocates `b` for max(count, min_count) elements first (DevBuf::alloc: detaches when shared)
    template <typename U>
    int upload(DevBuf& b, const U* src, size_t count, size_t min_count = 0) {
        HIPC(b.alloc(sizeof(U) * std::max(count, min_count)));
        return upload_to(b.p, src, count);
    }
    template <typename U>
    int download(U* dst, const void* src, size_t count) {
        if (count) HIPC(hipMemcpyAsync(dst, src, sizeof(U) * count, hipMemcpyDeviceToHost, stream));
        return SPFM_OK;
    }

    // Staged work of the read-only units: `enqueue` issues a call's copies and kernels on `stream`
    // and returns a status, this waits for them.  Every allocation comes first, in the caller:
    // once the staging copies are in flight, nothing returns before a sync -- host staging vectors
    // (and the caller's arrays) may still be read by a copy in flight, so on an error the stream
    // is synchronised all the same and the first error's message is kept.  After a clean sync the
    // timer is collected and its time added to *device_us (microseconds, saturating at 2e9).
    template <typename F>
    int run_staged(F&& enqueue, DeviceTimer* timer = nullptr, int* device_us = nullptr) {
        const int rc = enqueue();
        if (rc) {
            const std::string first = err;
            (void)sync();
            err = first;
            return rc;
        }
        SPFM_TRY(sync());  // staging and the caller's arrays are not read after this
        if (timer) timer->collect();
        if (timer && device_us) *device_us = (int)std::min(*device_us + timer->ms * 1e3, 2e9);
        return SPFM_OK;
    }

    // Rows [r0, r1) of a host CSR matrix into (rp, ri, rv), the values as T (the whole matrix:
    // r0 = 0).  indptr goes up unshifted: a kernel that is given a block r0 > 0 gets the entry
    // base indptr[r0] separately.  The entry buffers hold at least `min_entries` elements.  `hv`
    // is the conversion's staging and stays alive until the caller's next sync().
    template <typename T>
    int stage_csr_rows(DevBuf& rp, DevBuf& ri, DevBuf& rv, std::vector<T>& hv,
                       const int64_t* indptr, const int32_t* indices, const double* data,
                       int64_t r0, int64_t r1, size_t min_entries = 0) {
        // (whole matrix: entries from position 0 whatever indptr[0] says -- predict_csr does
        // not ask for indptr[0] == 0 and its kernels index by indptr as given)
        const int64_t e0 = r0 ? indptr[r0] : 0, ne = indptr[r1] - e0;
        const T* vals;
        if constexpr (std::is_same<T, double>::value) {
            vals = data + e0;
        } else {
            hv.resize((size_t)ne);
            const int nt = (ne >= (1 << 20)) ? schedule_threads() : 1;
            const int64_t per = (ne + nt - 1) / nt;
            auto work = [&](int tid) {
                const int64_t lo = per * tid, hi = std::min<int64_t>(ne, lo + per);
                for (int64_t ii = lo; ii < hi; ++ii) hv[(size_t)ii] = (T)data[e0 + ii];
            };
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; ++t) pool.emplace_back(work, t);
            work(0);
            for (auto& th : pool) th.join();
            vals = hv.data();
        }
        SPFM_TRY(upload(rp, indptr + r0, (size_t)(r1 - r0 + 1)));
        SPFM_TRY(upload(ri, indices + e0, (size_t)ne, min_entries));
        return upload(rv, vals, (size_t)ne, min_entries);
    }

    // the pairs (0, y_i) -- prediction and target of row i side by side -- into `yy`, which the
    // caller has allocated; `hy` stays alive until the caller's next sync()
    template <typename T>
    int upload_targets(const double* y, std::vector<T>& hy) {
        hy.resize((size_t)n * 2);
        for (int64_t i = 0; i < n; ++i) {
            hy[(size_t)2 * i] = (T)0;
            hy[(size_t)2 * i + 1] = (T)y[i];
        }
        return upload_to(yy.p, hy.data(), hy.size());
    }

    // Block `order_idx` of the live parameter image as element strides (component, feature):
    // (k,d) after pcd epochs and spfm_set_params, (d,k) after pbcd / psgd.
    struct BlockView {
        const double* base;
        int64_t ss, sj;
    };
    BlockView live_block(int order_idx) const {
        const double* img = p_valid ? P.as<double>() : Pt.as<double>();
        return {img + (size_t)order_idx * k * d, p_valid ? (int64_t)d : 1, p_valid ? 1 : (int64_t)k};
    }

    // ---------------------------------------------------------------- profiling
    // One event pair per recorded launch (bounded pool); launches beyond the pool
    // are not counted, so ms / launches / nnz always describe the same set.
    static constexpr size_t kProfPool = 32768;
    bool prof_armed = false;
    void prof_begin(int which, int64_t nnz_launch) {
        prof_armed = false;
        if (!prof_on) return;
        ProfSlot& ps = prof[which];
        if (ps.used + 2 > kProfPool) return;
        if (ps.used + 2 > ps.ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess) return;
            if (hipEventCreate(&b) != hipSuccess) {
                (void)hipEventDestroy(a);
                return;
            }
            ps.ev.push_back(a);
            ps.ev.push_back(b);
        }
        ps.launches++;
        ps.nnz += nnz_launch;
        (void)hipEventRecord(ps.ev[ps.used], stream);
        prof_armed = true;
    }
    void prof_cancel(int which, int64_t nnz_launch) {  // the launch announced by prof_begin was not made
        if (!prof_armed) return;
        prof[which].launches--;
        prof[which].nnz -= nnz_launch;
        prof_armed = false;
    }
    void prof_end(int which) {
        if (!prof_armed) return;
        ProfSlot& ps = prof[which];
        (void)hipEventRecord(ps.ev[ps.used + 1], stream);
        ps.used += 2;
        prof_armed = false;
    }
    void prof_collect() {
        if (!prof_on) return;
        (void)hipStreamSynchronize(stream);
        for (auto& ps : prof) {
            for (size_t i = 0; i + 1 < ps.used; i += 2) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, ps.ev[i], ps.ev[i + 1]) == hipSuccess) ps.ms += ms;
            }
            ps.used = 0;
        }
    }

    int64_t batch_nnz(int b) const {
        int64_t s = 0;
        for (int q = batch_ptr[b]; q < batch_ptr[b + 1]; ++q)
            s += h_cptr[order[q] + 1] - h_cptr[order[q]];
        return s;
    }

    int shm_barrier();

    int allreduce_shm(double* buf, size_t count);
    int allreduce_shm_piece(double* buf, size_t count);

    int allreduce(double* buf, size_t count);

    int ensure_col_norm();

    int ensure_p();
    int ensure_pt();

    // ---------------------------------------------------------------- graph util
    // Runs `body` (which only enqueues work on `stream`) either directly or, when
    // graphs are enabled, captured once under `key` and replayed.
    template <typename F>
    int run_cached(const std::string& key, F&& body) {
        const bool graph_ok = use_graph && !prof_on && !dist();
        if (!graph_ok) return body();
        auto it = graphs.find(key);
        if (it == graphs.end()) {
            hipGraph_t g = nullptr;
            HIPC(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            int rc = body();
            hipError_t e = hipStreamEndCapture(stream, &g);
            if (rc != SPFM_OK) {
                if (g) (void)hipGraphDestroy(g);
                return rc;
            }
            if (e != hipSuccess) {
                err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
                return SPFM_ERR_RUNTIME;
            }
            hipGraphExec_t ge = nullptr;
            e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) {
                err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
                return SPFM_ERR_RUNTIME;
            }
            it = graphs.emplace(key, ge).first;
        }
        HIPC(hipGraphLaunch(it->second, stream));
        return SPFM_OK;
    }

    template <typename T>
    int upload_images(const int64_t* h_cp, const int32_t* h_ci, const int64_t* h_rp,
                      const int32_t* h_ri, const double* data_csc, const double* data_csr,
                      const int64_t* perm, const double* y);

    template <typename T>
    int set_data_t(const int64_t* indptr, const int32_t* indices, const double* data,
                   const double* y);

    int data_installed(const double* y);

    // CSR ingest on the DEVICE (round 3; SURVEY.md 8f N4 as written): the CSR arrays go up once
    // (they are the engine's row-major image anyway), the CSC image is their stable radix sort
    // by column id (spfm_ingest.hip); the host keeps only the CSC *structure* (indptr, row ids),
    // copied back for the schedule and stream builders.  Returns kIngestFallback when the device
    // path cannot be used (the host-thread transposition then takes over).
    bool ingest_device = true;
    int ingest_device_used = 0;
    int co_tenants = 1;  // persistent passes of other handles expected on the device at the same time
    static constexpr int kIngestFallback = 2;
    template <typename T>
    int set_data_csr_device(const int64_t* indptr, const int32_t* indices, const double* data,
                            const double* y);

    int set_data_csr(int64_t n_, int32_t d_, const int64_t* indptr, const int32_t* indices,
                     const double* data, const double* y);

    int set_data(int64_t n_, int32_t d_, const int64_t* indptr, const int32_t* indices,
                 const double* data, const double* y);

    int set_params(int n_orders_, int k_, int32_t d_, const double* P_, const double* w_,
                   const double* lams_);

    int get_params(double* P_, double* w_);

    int configure(int solver_, int loss_, int reg_, int top_degree_);

    int alloc_work();

    // =============================================================== schedule
    // First-fit colouring of the conflict graph in the visiting order `jf` into order / batch_ptr:
    // on the device when the conflict structure is the handle's own matrix (spfm_colour.hip; the
    // same classes as the host form, tests/test_hip_colour.py), else -- global structure of a
    // sharded run, small problems, more than 4096 colours -- by the host threads.
    bool colour_device = true;
    int colour_device_used = 0;
    bool stream_device = true;   // the 64-column pass's entry stream built on the device
    int stream_device_used = 0;
    int pb_stream_device_used = 0, wide_stream_device_used = 0;  // the pbcd / wide entry streams
    // Test hook "debug_setup_any_size": the device colouring and the device stream builders run
    // whatever the problem's size (every other guard stays), and the builders keep what the
    // passes do not need but spfm_debug_stream_tables reads: the entries' CSC positions (and the
    // wide stream's flags and the relaxed runs' skip mask), which are otherwise freed once the
    // row / value images are gathered.
    bool debug_setup_any_size = false;
    DevBuf dbg_prb_src, dbg_r_src, dbg_pb_src, dbg_w_src, dbg_w_hz;
    std::vector<uint8_t> dbg_r_skip;
    int64_t dbg_r_entries = 0;   // entries of the relaxed runs' stream
    int relax_stream_device_used = 0;  // ... and whether the device built it
    int pb_stream_balance = 0;   // the slot map the pbcd stream was built with
    int debug_stream_info(int which, int64_t* info8);
    int debug_stream_tables(int which, int32_t* sp, int32_t* src, uint8_t* flags, uint32_t* lmask,
                            uint8_t* tab, uint8_t* skip, int32_t* batch_ptr_out);
    int colour_columns(int mode, int64_t rows, const int64_t* cp, const int32_t* ci, bool own,
                       const int32_t* jf, int max_batch);

    int set_schedule(int mode, const int32_t* indices_feature, const int64_t* cf_indptr,
                     const int32_t* cf_indices, int64_t cf_rows, int32_t* order_out,
                     int32_t* n_batches_out);

    int install_schedule();

    int set_schedule_raw(const int32_t* order_in, const int32_t* bptr_in, int32_t nb,
                         const int64_t* cf_indptr, const int32_t* cf_indices, int64_t cf_rows);

    int n_batches() const { return (int)batch_ptr.size() - 1; }

    template <typename T, int M>
    void launch_anova(int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv,
                      const double* Pt_o, double* out);
    template <typename T>
    int anova_dispatch(int kind, int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv,
                       const double* Pt_o, double* out);

    template <typename T>
    int output_t(int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv, int degree,
                 int fit_linear, int add_lower, double* out);

    template <typename T>
    int init_pred_t(int degree, int fit_linear, int add_lower);

    int init_pred(int degree, int fit_linear, int add_lower);

    template <typename T>
    int get_y_pred_t(double* out);

    template <typename T>
    int loss_sum_t(double* out);

    template <typename T>
    int predict_csr_t(int64_t rows, const int64_t* indptr, const int32_t* indices,
                      const double* data, int degree, int fit_linear, int add_lower,
                      double* out);

    int epoch_prologue();

    int epoch_epilogue(double* viol);

    static std::string fkey(const char* tag, std::initializer_list<double> v,
                            std::initializer_list<int64_t> iv) {
        std::string s(tag);
        char buf[64];
        for (double x : v) {
            snprintf(buf, sizeof buf, "|%a", x);
            s += buf;
        }
        for (int64_t x : iv) {
            snprintf(buf, sizeof buf, "|%lld", (long long)x);
            s += buf;
        }
        return s;
    }

    template <typename T>
    int lin_body(double alpha);

    template <typename T, int LOSS>
    int lin_prb(double alpha);
    template <typename T>
    int lin_prb_loss(double alpha);

    void mark_not_resident(const char* what) {
        pers_failed = true;
        pers_fallbacks += 1;
        pers_reason = std::string(what) + ": its workgroups cannot all be resident on this device";
        if (getenv("SPFM_VERBOSE")) fprintf(stderr, "spfm: fall-back: %s\n", pers_reason.c_str());
    }

    int cd_linear_epoch(double alpha, double* viol);

    template <typename T, int M>
    int pcd_pass_body(int order_idx, double beta, double gamma, double eta);

    // ---------------------------------------------------- persistent row-block pass
    // (several ranks: the persistent passes need the peer-mapped exchange slabs)
    bool prb_usable() const {
        return persistent && !pers_failed && (!dist() || peer_ready) && max_batch_cols <= 64 &&
               nnz < ((int64_t)1 << 31) && n > 0 && !weighted;
    }

    bool resident_ok(const void* fn, int threads, size_t lds, int G);
    static constexpr int kNotResident = 1;  // internal: the launch was not made, nothing changed
    int launch_groups(int G) {  // test hook: a launch that lacks its last workgroup times out
        if (debug_drop > 0 && G > 1) {
            --debug_drop;
            return G - 1;
        }
        return G;
    }
    int snapshot_state(const double* params, size_t count, DevBuf& dst);
    int persistent_aborted(bool* out);
    int recover_from_abort(double* params, size_t count, const DevBuf& src, const char* what);

    template <typename T>
    int ensure_prb();
    template <typename T>
    int build_prb_stream(int nb_);

    PrbArgs prb_args();

    // ---- relaxed runs for schedules of tiny steps (degree-2 pcd pass, one GPU)
    // worth trying: the persistent 64-column pass is in use and the strict steps are narrow
    bool relax_candidate() const {
        return relax_on && prb_usable() && !dist() && n_batches() > 0 &&
               (double)d / (double)n_batches() < 12.0 && !weighted;
    }
    template <typename T>
    int ensure_relax();
    PrbArgs relax_args();

    template <typename T, int M, int LOSS>
    int pcd_pass_prb(int order_idx, double beta, double gamma, double eta);

    template <typename T, int M>
    int pcd_prb_loss(int order_idx, double beta, double gamma, double eta);

    template <typename T>
    int pcd_prb_dispatch(int M, int order_idx, double beta, double gamma, double eta);

    int peer_clear(size_t off_doubles, size_t n_doubles);
    int host_barrier();

    // ------------------------------------------------------ wide persistent passes
    bool wide_usable() const {
        return persistent && !pers_failed && wide_on && (!dist() || peer_ready) &&
               max_batch_cols > 64 && max_batch_cols <= 512 && nnz < ((int64_t)1 << 31) && n > 0 &&
               !weighted;
    }

    int wide_groups(int ncu, size_t lds_max) const;

    template <typename T>
    int ensure_wide();

    PcdwArgs wide_args();

    template <typename T, int KIND>
    int wide_launch(PcdwArgs& a, PcdwParams& pp, T* Aptr);

    template <typename T>
    int pcd_pass_wide(int order_idx, double beta, double gamma, double eta);

    template <typename T>
    int lin_wide(double alpha);

    // template parameter for a reference degree: -1 (all-subsets) -> 0
    static int kind_of(int degree) { return degree == -1 ? 0 : degree; }
    bool degree_ok(int degree) const {
        return top_degree == -1 ? degree == -1 : (degree >= 2 && degree <= top_degree);
    }

    template <typename T, int M>
    int pcd_precompute_all(int order_idx);
    template <typename T>
    int pcd_precompute_all_dispatch(int M, int order_idx);

    template <typename T>
    int pcd_pass_dispatch(int M, int order_idx, double beta, double gamma, double eta);

    int pcd_epoch(int order_idx, int degree, double beta, double gamma, double eta,
                  const int32_t* ic, int n_comp, double* viol);

    template <typename T, int M, int L, int C>
    int pbcd_body_lc(int order_idx, double beta, double gamma, double eta);

    // ------------------------------------------------ persistent pbcd pass (one launch)
    static bool pbprb_degree_ok(int M) { return M == 0 || M == 2 || M == 3 || M == 4; }
    bool pbprb_usable(int M) const {
        return persistent && !pers_failed && pb_persistent && (!dist() || peer_ready) &&
               max_batch_cols <= 64 && nnz < ((int64_t)1 << 31) && n > 0 && k <= 62 &&
               pbprb_degree_ok(M) && !weighted;
    }

    const char* validate_pb_stream(int G, int NG, const std::vector<int32_t>& gsp,
                                   const std::vector<int32_t>& src,
                                   const std::vector<uint8_t>& meta,
                                   const std::vector<uint8_t>& tab) const;

    template <typename T>
    int ensure_pb_stream(int NG);
    template <typename T>
    int ensure_pb_relax(int NG);

    template <typename T, int M, int L>
    int pbcd_prb_l(int order_idx, double beta, double gamma, double eta);

    template <typename T, int M>
    int pbcd_prb_m(int order_idx, double beta, double gamma, double eta);

    template <typename T>
    int pbcd_prb_dispatch(int M, int order_idx, double beta, double gamma, double eta);

    template <typename T, int M>
    int pbcd_body(int order_idx, double beta, double gamma, double eta);

    template <typename T>
    int pbcd_dispatch(int M, int order_idx, double beta, double gamma, double eta);

    int pbcd_epoch(int order_idx, int degree, double beta, double gamma, double eta,
                   double* viol);

    // ================================================= host-stepped epochs
    // User-defined regularizer objects (regularizer/__init__.py:8-15, base.py:27-34: the
    // reference's duck-typed plug-in protocol) cannot run inside the device chains.  For them the
    // epoch is stepped from the host: per dependent step the device forms the column sums
    // (pcd.py:54-59 / pbcd.py:60-67), the caller applies the update rule with its own
    // prox_cd / prox_bcd and cache hooks in visiting order, the device scatter-updates
    // (pcd.py:124-133 / pbcd.py:135-144).  Two host round trips per step: a path that honours
    // the plug-in surface, not a fast one.  Multi-kernel kernels; with several ranks the sums are
    // all-reduced like any other step.
    int host_order = -1, host_degree = 0;
    std::vector<double> host_stage;

    int host_epoch_begin(int order_idx, int degree);
    template <typename T>
    int host_pbcd_precompute(int M, int order_idx);
    int host_pass_begin(int s);
    int host_step_check(int b) {
        if (host_order < 0) FAIL(SPFM_ERR_INVALID, "host step: call spfm_host_epoch_begin first");
        if (b < 0 || b >= n_batches()) FAIL(SPFM_ERR_INVALID, "host step: step index out of range");
        return SPFM_OK;
    }

    template <typename T, int M>
    int host_sums_pcd(int b, double* out);
    template <typename T, int M>
    int host_apply_pcd(int b, const double* p_new);
    template <typename T, int M, int L, int C>
    int host_sums_pbcd(int b, double* out);
    template <typename T, int M, int L, int C>
    int host_apply_pbcd(int b, const double* p_new, const double* p_old);
    // dispatch on (storage type, degree[, component lanes]) as the multi-kernel engine does
    template <typename T>
    int host_step_pcd_t(bool sums, int b, double* out, const double* p_new);
    template <typename T>
    int host_step_pbcd_t(bool sums, int b, double* out, const double* p_new, const double* p_old);
    int host_step(bool sums, int b, double* out, const double* p_new, const double* p_old);
    int host_epoch_end(double* viol);

    int configure_psgd(int loss_, int reg_, int top_degree_);

    // The psgd unit (spfm_engine_psgd.hip).  The pure host rules -- step sizes, the tabulated
    // epoch, the sharded lists, the sampler's CSR checks -- live in spfm_psgd_host.h; a PsgdStep
    // is filled once per extern "C" entry and handed down by reference.
    int psgd_ready(const char* what, int degree);  // data, parameters, configured for psgd
    template <typename S>
    void loss_sum(const S* src, int64_t n_items, int slot);  // scalar[slot] = sum src[0, n)
    int psgd_epoch_end(const double* loss_row, int64_t n_items, double* sum_loss);
    template <typename T, int L>
    int psgd_epoch_tl(const PsgdStep& st);
    // row_lo / n_samples: several ranks (spfm_psgd_epoch_sharded); one rank: 0 / n
    int psgd_epoch(const PsgdStep& st, const int32_t* indices_samples, int64_t n_samples,
                   int64_t row_lo, double* sum_loss);
    // several ranks: per minibatch of the GLOBAL order this rank's samples (first position in
    // its local sample list, count) and the global batch size (shard_batches)
    std::vector<int64_t> sg_lpos;
    std::vector<int32_t> sg_lB, sg_gB;
    // what follows a gradient launch, shared by the pointwise and the pairwise gradient
    template <int L, typename GradFn>
    int psgd_batches_tl(GradFn&& grad, const char* tag, int64_t tsize_, int64_t n_items,
                        const PsgdStep& st);
    // per-feature AdaGrad steps: handle state.  A_P (n_orders, d) and
    // A_w (d), sized at the setter (acc_orders, acc_d) and cleared by it alone; every epoch entry
    // of the unit takes the mode, G0 and the reason it cannot run through its PsgdStep
    DevBuf sg_accP, sg_accw;
    int psgd_adaptive = 0;
    double psgd_g0 = 1.0;
    int acc_orders = 0;
    int32_t acc_d = 0;
    PsgdStep psgd_step(int degree, double alpha, double beta, double gamma, double eta0, int lr,
                       double power_t, int64_t batch_size, int fit_linear, int64_t* it) const;
    int psgd_set_adaptive(int mode, double g0, const double* acc_P, const double* acc_w);
    int psgd_get_adaptive(double* acc_P, double* acc_w);

    // pairwise ranking fit: triples (anchor, plus, minus) of rows of the
    // handle's data [X; Z]; buffers of their own (sg_samples and pred_tmp are sized by n)
    DevBuf sg_triples, sg_lossrow, sg_ordered;
    int psgd_pairs_check(const char* what, int degree, const int32_t* triples, int64_t m);
    int pairs_reserve(int64_t m);  // sg_triples / sg_lossrow; a moved buffer clears the graphs
    template <typename T, int L, bool WT>
    int psgd_pairs_epoch_tl(const PsgdStep& st, int64_t m);
    int psgd_pairs_epoch(const PsgdStep& st, const int32_t* triples, int64_t m, double* sum_loss);
    // weighted triples: one double per slot of sg_triples, read by the
    // WT instances of the gradient kernel; a moved sg_weights clears the graphs
    DevBuf sg_weights;
    int weights_reserve(int64_t m);
    int psgd_pairs_epoch_weighted(const PsgdStep& st, const int32_t* triples,
                                  const double* weights, int64_t m, double* sum_loss);
    int psgd_pairs_eval(int degree, int fit_linear, const int32_t* triples, int64_t m,
                        double* sum_loss, int64_t* n_ordered);
    // what follows the checks and the filling of sg_triples: the batches and the loss sum
    // (weighted: the kernel reads sg_weights)
    int psgd_pairs_run(const PsgdStep& st, int64_t m, double* sum_loss, bool weighted = false);

    // negatives drawn on the device: the positives (context and
    // candidate of each, canonical CSR order) and the forbidden CSR, uploaded once per data set;
    // sg_triples filled by psgd_pair_sample_kernel is `sampled` until an upload overwrites it
    DevBuf sm_posrow, sm_posidx, sm_fptr, sm_fidx, sg_scores, sg_order;
    int64_t sm_nctx = 0, sm_ncand = 0, sm_npos = 0, sampled_m = 0;
    bool have_sampler = false, sampled = false;
    int psgd_pairs_set_sampler(int64_t n_ctx, int64_t n_cand, const int64_t* pos_ptr,
                               const int32_t* pos_idx, const int64_t* forb_ptr,
                               const int32_t* forb_idx);
    int psgd_pairs_sample(int degree, int64_t n_negatives, int64_t n_candidates,
                          int64_t max_draws, int64_t seed, int64_t epoch, const int32_t* order,
                          int32_t* triples_out, double* scores_out);
    int psgd_pairs_epoch_sampled(const PsgdStep& st, double* sum_loss);
    // the proposal table and the positives' weights live and die with the
    // sampler; `sampled_weighted`: the last sample call wrote sg_weights (positive weights, WARP)
    DevBuf sm_cum, sm_posw, sg_trials;
    uint32_t sm_cumW = 0;
    bool have_proposal = false, have_posw = false, sampled_weighted = false;
    int psgd_pairs_set_proposal(const uint32_t* cum, int64_t n_cand);
    int psgd_pairs_set_positive_weights(const double* wq, int64_t nnz);
    // both sample entries; warp: n_candidates is the number of trials
    int psgd_pairs_sample_any(bool warp, int degree, int64_t n_negatives, int64_t n_candidates,
                              int64_t max_draws, double margin, int64_t seed, int64_t epoch,
                              const int32_t* order, int32_t* triples_out, double* scores_out,
                              double* weights_out, int32_t* trials_out);

    // listwise fit: a positive and its n_negatives negatives are one
    // item, read from the grouped triples in sg_triples; what the last sample call used is
    // remembered (a sampled list epoch needs order == NULL and the same n_negatives)
    DevBuf sg_listorder;
    int64_t sampled_nneg = 0;
    bool sampled_slots = false;
    int psgd_lists_check(const char* what, int degree, const int32_t* triples, int64_t m,
                         int64_t n_negatives, int list_loss);
    template <typename T, int L>
    int psgd_lists_epoch_tl(const PsgdStep& st, int64_t n_lists, int M, int list_loss,
                            bool ordered);
    int psgd_lists_run(const PsgdStep& st, int64_t n_lists, int M, int list_loss, bool ordered,
                       double* sum_loss);
    int psgd_lists_epoch(const PsgdStep& st, const int32_t* triples, int64_t m,
                         int64_t n_negatives, int list_loss, double* sum_loss);
    int psgd_lists_epoch_sampled(const PsgdStep& st, int64_t n_negatives, int list_loss,
                                 const int32_t* list_order, double* sum_loss);
    int psgd_lists_eval(int degree, int fit_linear, const int32_t* triples, int64_t m,
                        int64_t n_negatives, int list_loss, double* sum_loss, int64_t* n_first);

    // ------------------------------- objective terms, held-out set (spfm_engine_objective.hip)
    // Read-only views of the live state: they use buffers of their own, neither of the
    // P / Pt validity flags changes, nothing an epoch reads is written.
    DevBuf obj_rec, obj_fin, obj_out;  // stage-1 records, per-component totals, the 8 slots
    DevBuf ev_rptr, ev_ridx, ev_rval, ev_y, ev_pred, ev_pt, ev_part;
    int64_t ev_n = 0;
    bool have_eval = false, ev_has_y = false;
    template <int M>
    int objective_launch(const double* base, int64_t ss, int64_t sj, int kk, int all_subsets,
                         int is_w);
    int objective_terms(int order_idx, int degree, double* out8);
    template <typename T>
    int set_eval_t(int64_t rows, const int64_t* indptr, const int32_t* indices,
                   const double* data, const double* y);
    int set_eval_csr(int64_t rows, int32_t d_, const int64_t* indptr, const int32_t* indices,
                     const double* data, const double* y);
    // output_t on a given (d,k) image of all orders (no P <-> Pt bookkeeping)
    template <typename T>
    int output_pt_t(int64_t rows, const int64_t* rp, const int32_t* ri, const T* rv, int degree,
                    int fit_linear, int add_lower, const double* Pt_all, double* out);
    int eval_loss(int degree, int fit_linear, int add_lower, double* loss_sum_out,
                  double* y_pred_out);

    // ------------------------------- selected interactions (spfm_engine_interactions.hip)
    // Read-only like the objective terms.  W = P_o^T diag(lams) P_o is consumed tile by tile in
    // registers; the buffers below are O(d_a k + tiles / 4096 + K), nothing is of size d_a^2.  They
    // are kept between calls and freed by spfm_set_params or the option "interaction_release".
    DevBuf int_flag, int_pos, int_ids, int_tot, int_tmp;  // compaction
    DevBuf int_A, int_B;                                  // packed active columns, diag(lams) applied
    DevBuf int_rec, int_rec2;                             // per-tile records and their reduction
    DevBuf int_hist, int_cnt, int_keys, int_vals, int_keys2, int_vals2;  // select / list
    DevBuf int_io, int_out;                               // values / block
    // per-feature views (spfm_engine_partners.hip): query image and ranks, per-tile row records
    // and the degree answers, strip lists and merged lists of a slab
    DevBuf int_pq, int_pqr, int_prec, int_pdeg, int_pon;
    SelBufs int_psel;
    int int_da = 0, int_kp = 0, int_T = 0;  // of the last compaction
    int int_tile_budget = 0;  // option "interaction_tile_budget": tiles per launch (0 = default)
    int int_dlim = 0;         // option "interaction_features": only features < this (0 = all)
    int int_launches = 0;     // tile launches of the last pass (option "interaction_launches")
    size_t interaction_scratch_bytes() const {
        return int_flag.bytes + int_pos.bytes + int_ids.bytes + int_tot.bytes + int_tmp.bytes +
               int_A.bytes + int_B.bytes + int_rec.bytes + int_rec2.bytes + int_hist.bytes +
               int_cnt.bytes + int_keys.bytes + int_vals.bytes + int_keys2.bytes +
               int_vals2.bytes + int_io.bytes + int_out.bytes + int_pq.bytes + int_pqr.bytes +
               int_prec.bytes + int_pdeg.bytes + int_psel.bytes() + int_pon.bytes;
    }
    int interaction_view(const char* what, int order_idx, BlockView* v);
    int interaction_prepare(const char* what, int order_idx);
    IntArgs interaction_args();
    void interaction_release();  // frees the scratch (set_params, option "interaction_release")
    int interaction_stats(int order_idx, double tol, int64_t* counts2, double* sums3);
    int interaction_topk(int order_idx, int64_t K, int32_t* rows, int32_t* cols, double* vals,
                         int64_t* n_out);
    int interaction_list(int order_idx, double tol, int64_t capacity, int32_t* rows,
                         int32_t* cols, double* vals, int64_t* n_out);
    int interaction_values(int order_idx, int64_t L, const int32_t* rows, const int32_t* cols,
                           double* vals);
    int interaction_block(int order_idx, int64_t nJ, const int32_t* J, int64_t nJ2,
                          const int32_t* J2, double* out);

    // per-feature views of W (spfm_engine_partners.hip): the full square,
    // query rows in slabs against candidate strips; scratch O(slab * tiles + slab * strips * K)
    int interaction_degrees(int order_idx, double tol, int64_t cand_strip, int64_t* degree,
                            double* sum_abs, double* max_abs, int32_t* strongest);
    int interaction_partners(int order_idx, int64_t nJ, const int32_t* J, int64_t K,
                             int32_t cand_lo, int32_t cand_hi, int by, int64_t row_slab,
                             int64_t cand_strip, int32_t* ids, double* vals, int32_t* n_out);

    // ------------------------------- third-order weights (same unit)
    // T[a, j, l] = sum_s lams_s p_sa p_sj p_sl over a < j < l, on the compaction, the packed images
    // and the scratch of the pair passes above (freed by the same three things); nothing of size
    // d_a^3 or d_a^2 is allocated.  A unit is (pair tile, pivot block); "interaction_tile_budget"
    // and "interaction_launches" count in units here.
    int interaction3_prepare(const char* what, int order_idx);  // + the work guard
    int interaction3_stats(int order_idx, double tol, int64_t* counts2, double* sums3);
    int interaction3_topk(int order_idx, int64_t K, int32_t* i, int32_t* j, int32_t* l,
                          double* vals, int64_t* n_out);
    int interaction3_list(int order_idx, double tol, int64_t capacity, int32_t* i, int32_t* j,
                          int32_t* l, double* vals, int64_t* n_out);
    int interaction3_values(int order_idx, int64_t L, const int32_t* i, const int32_t* j,
                            const int32_t* l, double* vals);

    // ------------------------------- the driver both orders go through: stats, select and list of
    // one compaction, written against an IntPass (what a pass over pairs or triples is)
    int interaction_run(const IntPass& ps, int mode, IntArgs a);  // a whole pass
    int interaction_run(const IntPass& ps, int mode, IntArgs a, int64_t u0, int64_t u1);
    int interaction_emit(const IntPass& ps, double tol, unsigned long long thr_key, int64_t cap,
                         int64_t* n_found);
    int interaction_pass_stats(const IntPass& ps, double tol, int64_t* counts2, double* sums3);
    int interaction_pass_topk(const IntPass& ps, int64_t K, int32_t* const* ids, double* vals,
                              int64_t* n_out);
    int interaction_pass_list(const IntPass& ps, double tol, int64_t capacity, int32_t* const* ids,
                              double* vals, int64_t* n_out);
    // IntPass::unpack: sorted keys -> the caller's id arrays (pairs: 2, triples: 3)
    int interaction_unpack(const uint64_t* keys, size_t n, int32_t* const* ids);
    int interaction3_unpack(const uint64_t* keys, size_t n, int32_t* const* ids);

    // ------------------------------- candidate ranking (spfm_engine_rank.hip)
    // score[b, c] = _get_output(x_b + z_c) for disjoint supports = rowconst + colconst + U V^T
    // (DESIGN.md section 15).  The candidate towers (rk_V, rk_cc) are built once by
    // rank_set_candidates and kept; contexts go through in slabs of rows.  Nothing is of size
    // n_ctx * n_cand.  Freed by spfm_set_params, spfm_destroy or spfm_rank_release.
    DevBuf rk_V, rk_cc;                    // candidate towers (padded rows, rk_Rp), constants
    DevBuf rk_U, rk_rc;                    // context towers of one slab
    DevBuf rk_xp, rk_xi, rk_xv;            // CSR staging (contexts or candidates)
    SelBufs rk_sel;                        // per-strip lists, merged lists of one slab
    DevBuf rk_dense;                       // dense scores of one slab
    DevBuf rk_ep, rk_ei;                   // excluded candidates of the call's rows (CSR pattern)
    DevBuf rk_tp, rk_ti, rk_ts, rk_tr;     // rank_eval: targets, their scores and counts
    DevBuf rk_pairs;                       // ... (row tile, candidate tile) pairs with a target
    std::vector<uint8_t> rk_zflag;         // columns with a stored candidate entry
    bool rk_have = false;
    int64_t rk_C = 0;
    int rk_R = 0, rk_Rp = 0, rk_degree = 0, rk_lin = 0, rk_lower = 0;
    int rk_row_slab = 0;    // spfm_rank_set_partition: context rows per slab (0 = default)
    int rk_cand_strip = 0;  // ... and candidates per strip (0 = default)
    int rk_device_us = 0;   // spfm_rank_info: kernels of the last scores / topk call
    size_t rank_scratch_bytes() const {
        return rk_V.bytes + rk_cc.bytes + rk_U.bytes + rk_rc.bytes + rk_xp.bytes + rk_xi.bytes +
               rk_xv.bytes + rk_sel.bytes() + rk_dense.bytes +
               rk_ep.bytes + rk_ei.bytes + rk_tp.bytes + rk_ti.bytes + rk_ts.bytes + rk_tr.bytes +
               rk_pairs.bytes;
    }
    void rank_release();  // frees the scratch and forgets the candidates
    // a caller's CSR rows before any device work: indptr starts at 0 and does not decrease, no
    // row longer than max_row_len, column ids in [0, d_)
    int check_csr(const char* what, int64_t rows, const int64_t* indptr, const int32_t* indices,
                  const double* data, int d_, int64_t max_row_len);
    template <int M>
    void rank_launch_tower(int64_t row0, int64_t rows, int order_idx, bool lin, int side, int col0,
                           double* img, double* cst);
    int rank_towers(int64_t row0, int64_t rows, int side, double* img, double* cst);
    int rank_set_candidates(int degree, int fit_linear, int add_lower, int64_t n_cand,
                            const int64_t* indptr, const int32_t* indices, const double* data);
    int rank_contexts(const char* what, int64_t n_ctx, const int64_t* indptr,
                      const int32_t* indices, const double* data);
    int rank_scores(int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                    const double* data, double* out);
    // (eptr NULL: nothing excluded, the selection spfm_rank_topk has always launched)
    int rank_topk(int64_t n_ctx, const int64_t* indptr, const int32_t* indices,
                  const double* data, const int64_t* eptr, const int32_t* eidx, int64_t K,
                  int32_t* idx_out, double* val_out, int64_t* k_out);
    int rank_check_pattern(const char* what, const char* name, int64_t rows, const int64_t* ptr,
                           const int32_t* idx);
    int rank_eval(int64_t n_ctx, const int64_t* indptr, const int32_t* indices, const double* data,
                  const int64_t* tptr, const int32_t* tidx, const int64_t* eptr,
                  const int32_t* eidx, int32_t* rank_out, double* score_out, int32_t* n_eff_out);

    // ------------------------------- per-row attributions (spfm_engine_explain.hip)
    // phi_ij (exact Shapley values against a zero baseline) or df/dx_ij on the stored entries of a
    // CSR matrix, their row sums and the per-row top-K.  Read-only like
    // predict; rows go through in slabs bounded by stored entries, the scratch below holds one slab
    // and is kept until spfm_set_params or spfm_destroy.
    DevBuf ex_rp, ex_ri, ex_rv;   // CSR image of one slab (values in the handle's precision)
    DevBuf ex_out, ex_rs;         // its values and row sums
    DevBuf ex_coef;               // the blocks' coefficient tables (n_blocks x k x 7)
    DevBuf ex_ti, ex_tv;          // its top-K lists
    static constexpr int64_t kExplainSlabMax = 1ll << 23;  // entries per slab: default and largest
    int64_t ex_slab_nnz = 0;      // spfm_explain_set_partition: stored entries per slab (0 = default)
    int64_t ex_slabs = 0;         // spfm_explain_info: slabs of the last call ...
    int ex_device_us = 0;         // ... and its kernels' device time
    size_t explain_scratch_bytes() const {
        return ex_rp.bytes + ex_ri.bytes + ex_rv.bytes + ex_out.bytes + ex_rs.bytes +
               ex_coef.bytes + ex_ti.bytes + ex_tv.bytes + ex_pp.bytes + ex_pv.bytes +
               ex_grp.bytes + ex_gp.bytes + ex_gm.bytes;
    }
    void explain_release();
    struct ExplainCall {  // the arguments of spfm_explain_csr / spfm_explain_topk_csr
        int64_t n;
        const int64_t* indptr;
        const int32_t* indices;
        const double* data;
        int n_blocks;
        const int32_t* order_idx;
        const int32_t* degree;
        const double* coef;
        int fit_linear, mode;
        double *out_vals, *out_rowsum;  // values: either may be NULL
        bool topk;                      // the top-K entry: K, idx, val (else K = 0)
        int K;
        int32_t* idx;
        double* val;
    };
    int explain_check(const char* what, const ExplainCall& c);
    // its two halves, shared with the pair entries: the parameters and blocks; the CSR rows
    int explain_check_model(const char* what, const ExplainCall& c);
    int explain_check_rows(const char* what, const ExplainCall& c);
    template <typename T, int M>
    void explain_launch_block(int64_t rows, int64_t e0, const double* Pt_o, const double* coef_o,
                              int mode);
    template <typename T>
    int explain_slab(const ExplainCall& c, int64_t r0, int64_t r1);
    template <typename T>
    int explain_run(const char* what, const ExplainCall& c);

    // ------------------------------- per-row pair attributions (spfm_engine_pairs.hip)
    // phi_iab (Shapley-Taylor index of order 2 against a zero baseline) or d2f/dx_ia dx_ib on the
    // stored pairs of every row, main_ia, the per-row top-K pairs and group x group tables
    // (DESIGN.md section 16a).  On the explain unit's slab image, coefficient upload, checks,
    // timing and partition; a slab additionally holds at most 2 slab_nnz pairs (2^24 at the
    // default).  Its scratch is counted and freed with the explain scratch.
    DevBuf ex_pp, ex_pv;          // pair offsets of one slab (rows + 1) and its pair values
    DevBuf ex_grp, ex_gp, ex_gm;  // group of every column (d); a slab's tables and grouped main
    enum { PAIRS_LIST = 0, PAIRS_TOPK = 1, PAIRS_GROUPED = 2 };  // the three entries
    struct PairsCall {
        ExplainCall m;  // rows and model; K / idx (first columns) / val of the top-K entry
        int kind;       // PAIRS_LIST ...
        int pmode;      // SPFM_PAIRS_INTERACTION / _HESSIAN
        int G;
        const int32_t* group;
        double *out_pairs, *out_main;
        int32_t* col_b;
    };
    int pairs_check(const char* what, const PairsCall& c);
    template <typename T, int M>
    void pairs_launch_block(int64_t rows, int64_t e0, const double* Pt_o, const double* coef_o,
                            int mode);
    template <typename T>
    int pairs_slab(const PairsCall& c, const int64_t* pp, int64_t r0, int64_t r1);
    template <typename T>
    int pairs_run(const char* what, const PairsCall& c);

    // ------------------------------- model banks (spfm_engine_bank.hip)
    // F fitted models stacked along the component axis, resident until spfm_bank_release, the next
    // spfm_bank_set or spfm_destroy (independent of spfm_set_params: the bank brings its own
    // parameters).  One pass over the rows of a CSR matrix gives every model's score; the argmax,
    // the loss sums and the weighted mean are formed on the device behind it (DESIGN.md section
    // 17).  Rows go through in slabs bounded by stored entries; the scratch holds one slab.
    DevBuf bk_pt, bk_lams, bk_w, bk_koff;  // the image: blocks x d x S, S, d x F, F + 1
    DevBuf bk_rp, bk_ri, bk_rv;            // CSR image of one slab (values in the handle's precision)
    DevBuf bk_sc;                          // its scores (rows x F)
    DevBuf bk_y, bk_wt, bk_part, bk_fin;   // targets of one slab, mean weights, loss partials, sums
    DevBuf bk_oi, bk_o0, bk_o1;            // per-row results of one slab
    DevBuf bk_gw, bk_gg, bk_gpart, bk_gacc;  // group sums: weights and ids of one slab, its partial
                                             // tables, the call's running Q x G x F table
    // spfm_bank_group_auc (spfm_engine_bank_auc.hip): allocated by
    // auc_begin, freed by auc_release when the call returns
    DevBuf bk_akey, bk_ameta, bk_arow, bk_aw;  // keys (F x n), class and group (F x n), 0..n-1, weights
    DevBuf bk_askey, bk_asrow, bk_atmp;        // sorted keys and rows of one batch, the sort's storage
    DevBuf bk_asets, bk_ablk, bk_aout;         // set masks, the walk's block records, its results
    DevBuf bk_cblk, bk_cout;  // spfm_bank_group_curve: its walk's block
                              // records and results, beside the scratch above
    int bk_abatch = 0;                         // members per sort batch of the call
    size_t bk_atmp_bytes = 0;                  // the sort's storage for n pairs
    bool bk_have = false, bk_lin = false;
    int bk_F = 0, bk_S = 0, bk_d = 0, bk_blocks = 0, bk_degree[2] = {0, 0};
    int64_t bk_slab_nnz = 0;               // spfm_bank_set_partition: stored entries per slab (0 = default)
    int64_t bk_slabs = 0, bk_launches = 0;  // spfm_bank_info: of the last call
    size_t bank_image_bytes() const {
        return bk_have ? bk_pt.bytes + bk_lams.bytes + bk_w.bytes + bk_koff.bytes : 0;
    }
    void bank_release();
    int bank_set(int32_t d_, int F, const int32_t* koff, int n_blocks, const int32_t* degree,
                 const double* Pt_bank, const double* lams_bank, const double* w_bank);
    struct BankCall {  // the arguments of spfm_bank_scores / _argmax / _losses / _mean / _group_sums
        int what;  // BANK_SCORES ...
        int64_t n;
        int32_t d;
        const int64_t* indptr;
        const int32_t* indices;
        const double* data;
        double* out;         // scores (n x F), best (n), loss sums (F) or mean (n)
        int32_t* idx;        // argmax
        double* runner;      // argmax
        int loss;            // losses
        const double* y;     // losses: (n) or (n x F)
        int per_model;       // losses
        const double* wt;    // mean: (F) or NULL = 1 / F
        const double* weight;    // group sums: (n) or NULL = 1.0
        const int32_t* group;    // group sums: (n) ids in [0, G) or NULL = all 0
        int G, Q;                // group sums
        const int32_t* metrics;  // group sums: (Q) SPFM_LOSS_* / SPFM_METRIC_* ids
        const uint32_t* sets;    // group auc: (F x U) bitmasks over the groups or NULL
        int U;                   // group auc
        int64_t* pairs;          // group auc: (F x U x 3) or NULL
        double* curve;           // group curve: (F x U x SPFM_BANK_CURVE_VALUES); out is its auc_out
        int64_t* counts;         // group curve: (F x U x SPFM_BANK_CURVE_COUNTS) or NULL
    };
    int bank_check(const char* what, const BankCall& c);
    template <typename T, int M>
    void bank_launch_block(int64_t rows, int64_t e0, int q, int first);
    template <typename T>
    int bank_slab(const BankCall& c, int64_t r0, int64_t r1, int64_t part0);
    template <typename T>
    int bank_run(const char* what, const BankCall& c);
    // group auc and group curve: the checks beyond bank_check and the call's scratch; the keys of
    // one slab behind its predict launches (enqueued, inside run_staged); sorts, walks and results
    // after the last.  A call is the curve's when c.curve is set; its c.out (the AUC table) may be NULL
    int auc_check(const char* what, const BankCall& c);
    int auc_begin(const BankCall& c);
    void auc_slab(const BankCall& c, int64_t r0, int64_t rows);
    int auc_finish(const BankCall& c);
    void auc_empty(const BankCall& c);
    void auc_release();

    // ------------------------------- fold-in of new columns (spfm_engine_foldin.hip)
    // With every other column fixed the model output is affine in the parameters of one column j:
    // f(x_i) = c_i + z_i . theta_j on the rows that store j.  Per target column a ridge-regularised
    // GLM in R = n_blocks k (+ 1) unknowns, solved by a damped Newton iteration, one workgroup
    // per column.  Read-only like explain; the target columns go through
    // in groups whose design matrix fits the scratch, which is kept until spfm_set_params or
    // spfm_destroy.
    DevBuf fi_rp, fi_ri, fi_rv;   // CSR image of one group's rows (values in the handle's precision)
    DevBuf fi_tp, fi_y;           // per row: position of the target entry in its row, target
    DevBuf fi_Z, fi_c;            // per row: its design row (R padded to 4) and offset
    DevBuf fi_cp;                 // per column of the group: first row (columns + 1)
    DevBuf fi_coef;               // the blocks' coefficient tables (n_blocks x k x 7)
    DevBuf fi_theta, fi_stat, fi_it;  // per column: theta (Rp), 3 doubles, 2 ints
    static constexpr int64_t kFoldinBudget = 256ll << 20;  // bytes of Z in one group
    int64_t fi_max_rows = 0;      // spfm_foldin_set_partition: rows per group (0 = the scratch)
    int64_t fi_groups = 0, fi_ignored = 0;  // spfm_foldin_info: of the last call ...
    int fi_device_us = 0;         // ... and its kernels' device time
    size_t foldin_scratch_bytes() const {
        return fi_rp.bytes + fi_ri.bytes + fi_rv.bytes + fi_tp.bytes + fi_y.bytes + fi_Z.bytes +
               fi_c.bytes + fi_cp.bytes + fi_coef.bytes + fi_theta.bytes + fi_stat.bytes +
               fi_it.bytes;
    }
    void foldin_release();
    struct FoldinCall {  // the arguments of spfm_foldin_csr
        ExplainCall m;   // rows and model
        const double* y;
        double offset;
        int loss;
        int64_t n_cols;
        const int32_t* cols;
        double alpha, beta;
        int max_iter;
        double tol;
        double* theta;
        int64_t* n_rows;
        int32_t *n_iter, *converged;
        double *grad_norm, *obj0, *obj1;
    };
    struct FoldinPlan {  // what the checks leave behind: the participating rows per column
        int R = 0, Rp = 0;
        std::vector<int64_t> cptr;  // (n_cols + 1) into rows
        std::vector<int64_t> rows;  // row ids, per column ascending
        std::vector<int32_t> tpos;  // position of the target entry in its row
    };
    int foldin_check(const char* what, const FoldinCall& c, FoldinPlan& plan);
    template <typename T, int M>
    void foldin_launch_design(int64_t rows, int q, const FoldinCall& c, int Rp);
    template <typename T>
    int foldin_group(const FoldinCall& c, const FoldinPlan& plan, int64_t c0, int64_t c1);
    template <typename T>
    int foldin_run(const char* what, const FoldinCall& c);

    // diagnostics that need kernels of one translation unit
    int debug_stream_probe(int64_t* bytes_out);  // spfm_engine_pcd.hip
    int debug_write_probe(int bytes, int64_t* bytes_out);
};

// The device branch counters (spfm_common.hip.h: g_branch_count) exist once per translation
// unit; spfm_debug_branch_counts adds the units' copies up.  Each unit that runs chains defines
// its accessor with SPFM_DEFINE_BRANCH_COUNTS(name): out[0..BR_COUNT) += the unit's counters.
#define SPFM_DEFINE_BRANCH_COUNTS(name)                                                          \
    hipError_t name(unsigned* out, int reset) {                                                  \
        unsigned v[spfm::BR_COUNT];                                                              \
        hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(spfm::g_branch_count), sizeof v);       \
        if (e != hipSuccess) return e;                                                           \
        for (int i = 0; i < spfm::BR_COUNT; ++i) out[i] += v[i];                                 \
        if (reset) {                                                                             \
            const unsigned zero[spfm::BR_COUNT] = {0};                                           \
            e = hipMemcpyToSymbol(HIP_SYMBOL(spfm::g_branch_count), zero, sizeof zero);          \
        }                                                                                        \
        return e;                                                                                \
    }
hipError_t spfm_branch_counts_pcd(unsigned* out, int reset);
hipError_t spfm_branch_counts_prb_f32(unsigned* out, int reset);
hipError_t spfm_branch_counts_prb_f64(unsigned* out, int reset);
hipError_t spfm_branch_counts_wide(unsigned* out, int reset);
hipError_t spfm_branch_counts_pbcd(unsigned* out, int reset);
hipError_t spfm_branch_counts_pbprb_f32(unsigned* out, int reset);
hipError_t spfm_branch_counts_pbprb_f64(unsigned* out, int reset);
