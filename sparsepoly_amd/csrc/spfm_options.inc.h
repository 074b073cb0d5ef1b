// spfm_options.inc.h -- the string-keyed options of spfm_set_option / spfm_get_option: one row
// per key.  Included by spfm_engine_core.hip only.  include/spfm.h documents the same keys
// (tests/test_options_host.py compares the two).  A row is
//   {"key", class, access, invalidation mask, "description"}
// with `access` one of flag(member), integer(member, lo, hi), readout(member); the irregular
// keys name the functions below: with_set / with_get replace one direction of a plain row,
// custom(set, get) is a row without a member.
#include <climits>
#include <cstring>

namespace {

enum OptClass { TUNING, DIAGNOSTIC, TEST_HOOK, READOUT };
enum OptKind { OPT_FLAG, OPT_INT, OPT_READONLY, OPT_CUSTOM };

struct OptAccess {
    OptKind kind;
    bool spfm_engine::*b;  // the member behind the key: a bool ...
    int spfm_engine::*i;   // ... or an int
    int lo, hi;            // OPT_INT: accepted range, inclusive
    int (*set)(spfm_engine*, int);   // irregular rows: called instead of the generic assignment
    int (*get)(spfm_engine*, int*);  // ... and instead of the generic read (OPT_CUSTOM: nullptr =
                                     // the key cannot be set / read)
};
struct OptRow {
    const char* key;
    OptClass cls;
    OptAccess a;
    unsigned inv;  // spfm_engine::kInv* bits applied after a successful set
    const char* doc;
};

constexpr int kMax = INT_MAX, kMin = INT_MIN;
constexpr OptAccess flag(bool spfm_engine::*m) { return {OPT_FLAG, m, nullptr, 0, 1, nullptr, nullptr}; }
constexpr OptAccess integer(int spfm_engine::*m, int lo, int hi) { return {OPT_INT, nullptr, m, lo, hi, nullptr, nullptr}; }
constexpr OptAccess readout(bool spfm_engine::*m) { return {OPT_READONLY, m, nullptr, 0, 0, nullptr, nullptr}; }
constexpr OptAccess readout(int spfm_engine::*m) { return {OPT_READONLY, nullptr, m, 0, 0, nullptr, nullptr}; }
constexpr OptAccess custom(int (*set)(spfm_engine*, int), int (*get)(spfm_engine*, int*)) { return {OPT_CUSTOM, nullptr, nullptr, 0, 0, set, get}; }
constexpr OptAccess with_set(OptAccess a, int (*set)(spfm_engine*, int)) { return a.set = set, a; }
constexpr OptAccess with_get(OptAccess a, int (*get)(spfm_engine*, int*)) { return a.get = get, a; }

constexpr unsigned G = spfm_engine::kInvGraphs, PRB = spfm_engine::kInvPrbStream | G,
                   PB = spfm_engine::kInvPbStream | G, WIDE = spfm_engine::kInvWideStream | G,
                   RELAX = spfm_engine::kInvRelax | G, PBRELAX = spfm_engine::kInvPbRelax | G,
                   SCHED = spfm_engine::kInvSchedule | G;

// ---- the irregular keys
int set_co_tenants(spfm_engine* h, int value) {  // concurrent fits: handles sharing the device's CUs
    if (value < 1 || value > 64) {
        h->err = "co_tenants must be in [1, 64]";
        return SPFM_ERR_INVALID;
    }
    h->co_tenants = value;
    // every tenant keeps to its share of the CUs (one persistent workgroup per CU)
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device);
    const int share = std::max(1, ncu / value);
    if (h->prb_G > share) {
        h->prb_G = share;
        h->invalidate(spfm_engine::kInvPrbStream | spfm_engine::kInvRelax);
    }
    if (h->pbprb_G > share) {
        h->pbprb_G = share;
        h->invalidate(spfm_engine::kInvPbStream);
    }
    return SPFM_OK;  // the row's mask: the wide pass caps itself (wide_groups)
}
int set_peer_exchange(spfm_engine* h, int value) {
    // 0: give the in-kernel cross-GPU exchange up (a rank could not map its peers): the
    // passes fall back to the per-step collective.  (1 is set by spfm_peer_connect only.)
    if (value != 0) {
        h->err = "peer_exchange: only 0 can be set; connect with spfm_peer_connect";
        return SPFM_ERR_INVALID;
    }
    h->peer_ready = false;
    return SPFM_OK;
}
int set_pbprb_owners(spfm_engine* h, int value) {
    if (value != 0) {
        h->err = "pbprb_owners: dedicated owner workgroups were removed (only 0 is accepted)";
        return SPFM_ERR_UNSUPPORTED;
    }
    return SPFM_OK;
}
int get_pbprb_owners(spfm_engine*, int* v) { return *v = 0, SPFM_OK; }
int do_interaction_release(spfm_engine* h, int) { return h->interaction_release(), SPFM_OK; }
int get_persistent_active(spfm_engine* h, int* v) {
    return *v = h->have_schedule && (h->prb_usable() || h->wide_usable()), SPFM_OK;
}
int get_wide_active(spfm_engine* h, int* v) { return *v = h->have_schedule && h->wide_usable(), SPFM_OK; }
int get_relax_steps(spfm_engine* h, int* v) {
    *v = h->relax_state == 1 ? (int)h->r_batch_ptr.size() - 1
                             : (h->pbr_state == 1 ? (int)h->pbr_batch_ptr.size() - 1 : 0);
    return SPFM_OK;
}
int get_n_ranks(spfm_engine* h, int* v) { return *v = h->dist() ? h->n_ranks : 1, SPFM_OK; }
int get_pcdw_groups(spfm_engine* h, int* v) {  // 0 = not chosen yet
    return *v = h->wide_ready ? h->wide_G : h->pcdw_G, SPFM_OK;
}
int get_interaction_scratch_kib(spfm_engine* h, int* v) {
    return *v = (int)((h->interaction_scratch_bytes() + 1023) / 1024), SPFM_OK;
}
int get_free_mem_mib(spfm_engine* h, int* v) {  // hipMemGetInfo of the handle's device
    size_t fr = 0, tot = 0;
    if (hipSetDevice(h->device) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) {
        h->err = "hipMemGetInfo failed";
        return SPFM_ERR_RUNTIME;
    }
    return *v = (int)(fr >> 20), SPFM_OK;
}

#define M(name) &spfm_engine::name
const OptRow kOptions[] = {
    // ---- tuning: engine choice and launch shape
    {"use_graph", TUNING, flag(M(use_graph)), G, "hipGraph replay of the per-pass launch sequences"},
    {"fuse_chain", TUNING, flag(M(fuse_chain)), G, "fused chain+sync kernel for steps of <= 64 columns"},
    {"max_batch", TUNING, integer(M(max_batch_opt), 1, kMax), G, "columns per dependent step of the next coloured schedule"},
    {"persistent", TUNING, flag(M(persistent)), PRB, "one persistent launch per pcd component pass"},
    {"prb_groups", TUNING, integer(M(prb_G), 1, kMax), PRB | RELAX, "workgroups of the 64-column persistent pass"},
    {"prb_long", TUNING, integer(M(prb_long), 16, kMax), PRB | RELAX, "entries per (workgroup, step, slot) above which a slot is long"},
    {"prb_lds", TUNING, flag(M(prb_lds)), G, "keep the row block in LDS when it fits"},
    {"prb_pack", TUNING, flag(M(prb_pack)), G, "packed row records for degree-3 passes with rows in global memory"},
    {"relax", TUNING, flag(M(relax_on)), RELAX | PBRELAX, "merged steps for schedules of tiny steps"},
    {"pbcd_persistent", TUNING, flag(M(pb_persistent)), G, "the persistent pbcd pass"},
    {"pbprb_groups", TUNING, integer(M(pbprb_G), 1, kMax), PB | PBRELAX, "workgroups of the persistent pbcd pass"},
    {"pbprb_balance", TUNING, flag(M(pb_balance)), PB, "balanced slot groups of the persistent pbcd pass"},
    {"pbprb_owners", TUNING, custom(set_pbprb_owners, get_pbprb_owners), G, "dedicated owner workgroups: removed, only 0 is accepted"},
    {"pbcd_fuse", TUNING, flag(M(pbcd_fuse)), G, "multi-kernel pbcd: prep + chain in one launch"},
    {"wide", TUNING, flag(M(wide_on)), G, "the wide passes (steps of up to 512 columns)"},
    {"wide_min_cols", TUNING, integer(M(wide_min_cols), kMin, kMax), G, "mean class width below which 64-column steps are used"},
    {"pcdw_groups", TUNING, with_get(integer(M(pcdw_G), 1, kMax), get_pcdw_groups), WIDE, "workgroups of the wide pass (reads the count in use once its stream exists)"},
    {"wide_lds_rows", TUNING, integer(M(wide_lds_cap), kMin, kMax), G, "wide pass, block too large for LDS: rows of it kept there"},
    {"wide_ep", TUNING, flag(M(wide_ep)), G, "wide pass, rows in global memory: entry-parallel form"},
    {"wide_rec8", TUNING, flag(M(wide_rec8)), G, "wide pass: 8-byte (A, residual) row records where they apply"},
    {"ingest_device", TUNING, flag(M(ingest_device)), G, "CSR -> CSC on the device, else by host threads"},
    {"colour_device", TUNING, flag(M(colour_device)), G, "first-fit colouring on the device, else by host threads"},
    {"stream_device", TUNING, flag(M(stream_device)), PRB | PB | WIDE, "entry streams built on the device, else by host threads"},
    {"co_tenants", TUNING, with_set(integer(M(co_tenants), 1, 64), set_co_tenants), WIDE, "handles whose persistent passes share the device: caps prb_groups and pbprb_groups"},
    {"peer_exchange", TUNING, with_set(flag(M(peer_ready)), set_peer_exchange), SCHED | PRB | PB | WIDE, "0: give the in-kernel cross-GPU exchange up"},
    {"persistent_failed", TUNING, flag(M(pers_failed)), G, "0: try the persistent passes again after a fall-back"},
    {"psgd_eager", TUNING, flag(M(psgd_force_eager)), G, "launch every psgd minibatch eagerly"},
    {"psgd_graph_sweeps", TUNING, integer(M(psgd_graph_sweeps), 0, 64), G, "support-search sweeps recorded per psgd minibatch"},
    // the interaction passes are read-only views: their options leave the
    // captured graphs and every engine choice alone
    {"interaction_tile_budget", TUNING, integer(M(int_tile_budget), 0, kMax), 0, "tiles per launch of an interaction pass (0 = default)"},
    {"interaction_features", TUNING, integer(M(int_dlim), 0, kMax), 0, "interaction passes see only features below this (0 = all)"},
    {"interaction_release", TUNING, custom(do_interaction_release, nullptr), 0, "action: free the interaction passes' scratch"},
    // ---- diagnostics
    {"prb_stamps", DIAGNOSTIC, flag(M(prb_stamp_on)), G, "phase timers of the 64-column pass"},
    {"pcdw_stamps", DIAGNOSTIC, flag(M(wide_stamp_on)), G, "phase timers of the wide pass"},
    {"pbprb_stamps", DIAGNOSTIC, flag(M(pb_stamp_on)), G, "phase timers of the persistent pbcd pass"},
    {"pbprb_dbg", DIAGNOSTIC, integer(M(pb_dbg), kMin, kMax), G, "bit mask of the persistent pbcd pass's diagnostic counters"},
    {"probe_xcd", DIAGNOSTIC, integer(M(probe_xcd), kMin, kMax), G, "spfm_debug_exchange_cost on one XCD"},
    {"probe_lds", DIAGNOSTIC, integer(M(probe_lds), kMin, kMax), G, "LDS bytes per workgroup of spfm_debug_exchange_cost"},
    // ---- test hooks
    {"debug_spin_max", TEST_HOOK, integer(M(spin_max), 64, kMax), G, "polls of one in-kernel wait before a persistent pass gives up"},
    {"debug_drop_group", TEST_HOOK, integer(M(debug_drop), kMin, kMax), G, "the next N persistent launches lack their last workgroup"},
    {"debug_keep_last_error", TEST_HOOK, flag(M(keep_last_error)), G, "spfm_comm_init keeps the thread's stale HIP error"},
    {"debug_setup_any_size", TEST_HOOK, flag(M(debug_setup_any_size)), SCHED | PRB | PB | WIDE | RELAX | PBRELAX, "device colouring and device entry streams whatever the problem's size"},
    // ---- read-outs
    {"persistent_active", READOUT, custom(nullptr, get_persistent_active), 0, "the next pcd epoch uses a persistent pass"},
    {"wide_active", READOUT, custom(nullptr, get_wide_active), 0, "the next pcd epoch uses the wide pass"},
    {"pbprb_active", READOUT, readout(M(pbprb_active)), 0, "what the last pbcd epoch used"},
    {"prb_lds_active", READOUT, readout(M(prb_lds_active)), 0, "last pcd pass: 0 global rows, 1 LDS residual, 2 LDS prediction + sign"},
    {"prb_pack_active", READOUT, readout(M(prb_pack_active)), 0, "the last pcd pass used packed row records"},
    {"wide_lds_active", READOUT, readout(M(wide_lr_active)), 0, "last wide pass: 0 global rows, 1 all rows in LDS, 2 first rows of a block"},
    {"wide_ep_active", READOUT, readout(M(wide_ep_active)), 0, "the last wide pass used the entry-parallel form"},
    {"relax_steps", READOUT, custom(nullptr, get_relax_steps), 0, "merged steps per sweep (0 = strict steps)"},
    {"pb_relax_active", READOUT, readout(M(pb_relax_active)), 0, "the last pbcd epoch ran relaxed runs"},
    {"persistent_fallbacks", READOUT, readout(M(pers_fallbacks)), 0, "epochs redone on the multi-kernel engine"},
    {"psgd_redone", READOUT, readout(M(psgd_redone)), 0, "psgd epochs redone eagerly from a snapshot"},
    {"n_ranks", READOUT, custom(nullptr, get_n_ranks), 0, "ranks of the attached communicator"},
    {"peer_ready", READOUT, readout(M(peer_ready)), 0, "in-kernel cross-GPU exchange connected and verified"},
    {"ingest_device_used", READOUT, readout(M(ingest_device_used)), 0, "the last spfm_set_data_csr transposed on the device"},
    {"colour_device_used", READOUT, readout(M(colour_device_used)), 0, "the last coloured schedule was coloured on the device"},
    {"stream_device_used", READOUT, readout(M(stream_device_used)), 0, "64-column entry stream: 0 host, 1 device, 2 taken from a co-tenant"},
    {"pb_stream_device_used", READOUT, readout(M(pb_stream_device_used)), 0, "the pbcd entry stream was built on the device"},
    {"wide_stream_device_used", READOUT, readout(M(wide_stream_device_used)), 0, "the wide entry stream was built on the device"},
    {"interaction_launches", READOUT, readout(M(int_launches)), 0, "tile launches of the last interaction pass"},
    {"interaction_scratch_kib", READOUT, custom(nullptr, get_interaction_scratch_kib), 0, "scratch the interaction passes hold"},
    {"free_mem_mib", READOUT, custom(nullptr, get_free_mem_mib), 0, "free memory of the handle's device"},
};
#undef M

const OptRow* find_option(spfm_engine* h, const char* key) {
    for (const OptRow& r : kOptions)
        if (std::strcmp(r.key, key) == 0) return &r;
    h->err = std::string("unknown option: ") + key;
    return nullptr;
}
}  // namespace

int spfm_set_option(spfm_handle h, const char* key, int value) {
    if (!h || !key) return SPFM_ERR_INVALID;
    const OptRow* r = find_option(h, key);
    if (!r) return SPFM_ERR_INVALID;
    const OptAccess& a = r->a;
    if (a.set) {
        const int rc = a.set(h, value);
        if (rc != SPFM_OK) return rc;
    } else if (a.kind == OPT_FLAG) {
        h->*a.b = value != 0;
    } else if (a.kind == OPT_INT) {
        if (value < a.lo || value > a.hi) {
            h->err = std::string(key) + " must be in [" + std::to_string(a.lo) + ", " +
                     std::to_string(a.hi) + "]";
            return SPFM_ERR_INVALID;
        }
        h->*a.i = value;
    } else {  // a read-out
        h->err = std::string("unknown option: ") + key;
        return SPFM_ERR_INVALID;
    }
    h->invalidate(r->inv);
    return SPFM_OK;
}

int spfm_get_option(spfm_handle h, const char* key, int* value) {
    if (!h || !key || !value) return SPFM_ERR_INVALID;
    const OptRow* r = find_option(h, key);
    if (!r) return SPFM_ERR_INVALID;
    if (r->a.get) return r->a.get(h, value);
    if (r->a.b) {
        *value = h->*r->a.b;
    } else if (r->a.i) {
        *value = h->*r->a.i;
    } else {  // an action
        h->err = std::string("unknown option: ") + key;
        return SPFM_ERR_INVALID;
    }
    return SPFM_OK;
}
