// spfm_psgd_plan.hip.h -- what the two deterministic plans share on the host (DESIGN.md sections
// 19e and 19f): from enumerated (minibatch, column) keys to the tables of the runs.  The pointwise
// plan (det_plan, rows of the visiting order) and the triple plan (pairs_det_plan_t, three rows
// per triple) differ in how the entries are counted, enumerated and gathered, and in the list
// they compare; those come in as callables.
#pragma once
#include "spfm_engine.hip.h"
#include "spfm_psgd_det.hip.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

// the buffers of one plan (members of the handle); rec / recx hold rec_bytes / x_bytes per record
struct DetPlanBufs {
    DevBuf &keys, &vals, &entq, &rec, &recx, &segptr, &segcol, &bseg, &tmp, &figs;
};

// Sort N entries by key = minibatch * d + column (stable) and build seg_ptr / seg_col / bseg_ptr.
//   t1                         temporary bytes `lengths` needs of b.tmp
//   lengths()                  enqueues whatever the enumeration reads (N > 0 only)
//   enumerate(key, val, entq)  enqueues the kernel that writes key / value / position per entry
//   head(key, val, entq, flag) enqueues the kernel that gathers the records in sorted order and
//                              flags the head of every run
// b.figs: [0] runs, [1] longest run (read back into nseg / longest), [2] the callers' own.
// A moved table clears the graphs.  Ends in a stream synchronise.
template <typename LenFn, typename EnumFn, typename HeadFn>
int spfm_engine::det_plan_runs(DetPlanBufs b, size_t rec_bytes, size_t x_bytes, int64_t N,
                               int64_t nbat, size_t t1, LenFn&& lengths, EnumFn&& enumerate,
                               HeadFn&& head, int64_t& nseg, int64_t& longest) {
    using namespace spfm;
    int* h_figs = reinterpret_cast<int*>(h_scalar + 4);
    int* figs = b.figs.as<int>();
    const size_t nz = (size_t)(N > 0 ? N : 1);
    const void* old[] = {b.rec.p, b.recx.p, b.segptr.p, b.segcol.p, b.bseg.p};
    HIPC(b.keys.alloc(sizeof(uint64_t) * 2 * nz));  // the sort's double buffer; the first half
    HIPC(b.vals.alloc(sizeof(uint32_t) * 2 * nz));  // holds flags and segment ids afterwards
    HIPC(b.entq.alloc(sizeof(int32_t) * nz));
    HIPC(b.rec.alloc(rec_bytes * nz));
    HIPC(b.recx.alloc(x_bytes * nz));
    HIPC(b.segptr.alloc(sizeof(int32_t) * (nz + 1)));
    HIPC(b.segcol.alloc(sizeof(int32_t) * nz));
    HIPC(b.bseg.alloc(sizeof(int32_t) * ((size_t)nbat + 1)));
    const void* now[] = {b.rec.p, b.recx.p, b.segptr.p, b.segcol.p, b.bseg.p};
    if (memcmp(old, now, sizeof old) != 0) clear_graphs();
    uint64_t* kin = b.keys.as<uint64_t>();
    uint64_t* kout = kin + nz;
    uint32_t* vin = b.vals.as<uint32_t>();
    uint32_t* vout = vin + nz;
    int32_t* flag = reinterpret_cast<int32_t*>(kin);  // (free once the sort has read its input)
    int32_t* sid1 = flag + nz;
    // the key bits that can differ: minibatch * d + column < nbat * d
    const uint64_t kmax = (uint64_t)nbat * (uint64_t)d;
    unsigned bits = 1;
    while (bits < 64 && (kmax - 1) >> bits) ++bits;
    size_t t2 = 0, t3 = 0;
    HIPC(rocprim::radix_sort_pairs(nullptr, t2, kin, kout, vin, vout, nz, 0u, bits, stream));
    HIPC(rocprim::inclusive_scan(nullptr, t3, flag, sid1, nz, rocprim::plus<int32_t>(), stream));
    HIPC(b.tmp.alloc(std::max(t1, std::max(t2, t3))));
    HIPC(hipMemsetAsync(figs, 0, sizeof(int) * 4, stream));
    HIPC(hipMemsetAsync(b.bseg.p, 0, sizeof(int32_t) * ((size_t)nbat + 1), stream));
    HIPC(hipMemsetAsync(b.segptr.p, 0, sizeof(int32_t), stream));  // (no entry at all: no segment)
    if (N > 0) {
        SPFM_TRY(lengths());
        enumerate(kin, vin, b.entq.as<int32_t>());
        t2 = b.tmp.bytes;
        HIPC(rocprim::radix_sort_pairs(b.tmp.p, t2, kin, kout, vin, vout, (size_t)N, 0u, bits,
                                       stream));
        head(kout, vout, b.entq.as<int32_t>(), flag);
        t3 = b.tmp.bytes;
        HIPC(rocprim::inclusive_scan(b.tmp.p, t3, flag, sid1, (size_t)N,
                                     rocprim::plus<int32_t>(), stream));
        hipLaunchKernelGGL(det_seg_kernel, dim3(cdiv(N, kBlock)), dim3(kBlock), 0, stream, kout,
                           flag, sid1, N, d, nbat, b.segptr.as<int32_t>(),
                           b.segcol.as<int32_t>(), b.bseg.as<int32_t>(), figs);
        hipLaunchKernelGGL(det_longest_kernel, dim3(cdiv(N, kBlock)), dim3(kBlock), 0, stream,
                           b.segptr.as<int32_t>(), N, figs);
    }
    HIPC(hipGetLastError());
    SPFM_TRY(download(h_figs, figs, 2));
    HIPC(hipStreamSynchronize(stream));
    nseg = h_figs[0];
    longest = h_figs[1];
    return SPFM_OK;
}
