// spfm_colour.hip -- the first-fit colouring of the column conflict graph on the device
// (the schedule product; host form: spfm_schedule.cpp
// schedule_colored_parallel, whose rounds this file restates for the GPU).
//
// Two columns conflict when they share a row.  The sequential first fit visits the columns in
// the given order and gives each the lowest colour that none of its rows holds yet and whose class
// is not full (max_batch columns).  Rounds of kRound columns, exactly as on the host:
//   (1) snapshot  one workgroup per column of the round collects the colours present in its rows
//                 as of the START of the round (per-row colour lists, LDS bitmap of 4096 colours);
//   (2) conflicts which columns of the round share a row: (1) also enters every column into its
//                 rows' lists of round members; a second pass over the same rows pairs up the
//                 members of every row (a row is touched by more than one column of a round in
//                 under 1 % of the cases; merging the 32 k pairs' row lists would cost more than
//                 the whole colouring);
//   (3) resolve   ONE workgroup walks the round in order: column q takes the lowest colour outside
//                 its snapshot set, not full, and not held by an earlier column of the round that
//                 shares a row with it -- what the sequential loop would have chosen;
//   (4) commit    the columns append their colour to their rows' lists.
// All launches of all rounds are queued on the stream without a host round trip; the result is
// the colour of every visiting position.  More than 4096 colours: *overflow, the host form takes
// over.  Identical to the host colouring for every input (tests/test_hip_colour.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace spfm {

constexpr int kRound = 256;        // columns per round = threads of the resolving workgroup
constexpr int kColourWords = 64;   // 4096 colours

__global__ __launch_bounds__(256) void colour_snapshot_kernel(
    int nq, int head, const int32_t* __restrict__ order, const int64_t* __restrict__ cptr,
    const int32_t* __restrict__ cidx, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ rcnt, const int32_t* __restrict__ rcol,
    int32_t* __restrict__ rmcnt, int32_t* __restrict__ rmem,
    const unsigned long long* __restrict__ full, unsigned long long* __restrict__ F) {
    __shared__ unsigned long long u[kColourWords];
    const int q = blockIdx.x;
    if (q >= nq) return;
    if (threadIdx.x < kColourWords) u[threadIdx.x] = full[threadIdx.x];
    __syncthreads();
    const int32_t j = order[head + q];
    const int64_t cb = cptr[j], ce = cptr[j + 1];
    for (int64_t ii = cb + threadIdx.x; ii < ce; ii += blockDim.x) {
        const int32_t i = cidx[ii];
        const int32_t cnt = rcnt[i];
        const int64_t rb = rptr[i];
        rmem[rb + atomicAdd(&rmcnt[i], 1)] = q;  // member of the round on this row
        const int32_t* rc = rcol + rb;
        for (int32_t t = 0; t < cnt; ++t) {
            const int32_t c = rc[t];
            atomicOr(&u[c >> 6], 1ull << (c & 63));
        }
    }
    __syncthreads();
    if (threadIdx.x < kColourWords) F[(size_t)q * kColourWords + threadIdx.x] = u[threadIdx.x];
}

// conf[q][p >> 6] bit (p & 63), p < q: the round's columns q and p share a row
__global__ __launch_bounds__(256) void colour_conflict_kernel(
    int nq, int head, const int32_t* __restrict__ order, const int64_t* __restrict__ cptr,
    const int32_t* __restrict__ cidx, const int64_t* __restrict__ rptr,
    const int32_t* __restrict__ rmcnt, const int32_t* __restrict__ rmem,
    unsigned long long* __restrict__ conf) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int32_t j = order[head + q];
    const int64_t cb = cptr[j], ce = cptr[j + 1];
    for (int64_t ii = cb + threadIdx.x; ii < ce; ii += blockDim.x) {
        const int32_t i = cidx[ii];
        const int32_t cnt = rmcnt[i];
        if (cnt < 2) continue;
        const int32_t* rm = rmem + rptr[i];
        for (int32_t t = 0; t < cnt; ++t) {
            const int32_t p = rm[t];
            if (p < q) atomicOr(&conf[(size_t)q * (kRound / 64) + (p >> 6)], 1ull << (p & 63));
        }
    }
}

// state[0] = overflow flag, state[1] = classes in use.  The walk over the round is ONE WAVE: lane w
// holds word w of the 4096-colour bitmaps, so a column costs a few LDS round trips and a ballot
// and no workgroup barrier (a first version with 256 threads and three barriers per column spent
// 1.9 us per column, 0.48 ms per round -- 90 % of the whole colouring).
__global__ __launch_bounds__(kRound) void colour_resolve_kernel(
    int nq, int head, int max_batch, const unsigned long long* __restrict__ F_in,
    unsigned long long* __restrict__ conf, unsigned long long* __restrict__ full,
    int32_t* __restrict__ class_size, int32_t* __restrict__ colour_out,
    int32_t* __restrict__ round_colour, int* __restrict__ state) {
    extern __shared__ unsigned long long lds[];
    unsigned long long* F = lds;                                    // [kRound][kColourWords]
    unsigned long long* cf = F + (size_t)kRound * kColourWords;     // [kRound][kRound / 64]
    unsigned long long* extra = cf + (size_t)kRound * (kRound / 64);  // [kColourWords] scratch
    int* col = reinterpret_cast<int*>(extra + kColourWords);          // [kRound]
    int* cs = col + kRound;                                           // [4096] class sizes
    const int tid = threadIdx.x;
    for (int x = tid; x < kColourWords * 64; x += kRound) cs[x] = class_size[x];
    for (int x = tid; x < nq * kColourWords; x += kRound) F[x] = F_in[x];
    for (int x = tid; x < nq * (kRound / 64); x += kRound) {
        cf[x] = conf[x];
        conf[x] = 0ull;  // clean for the next round
    }
    if (tid < kColourWords) extra[tid] = 0ull;
    __syncthreads();
    if (state[0]) return;  // an earlier round overflowed: nothing more to do (uniform)
    if (tid >= 64) return;  // the walk is wave 0's
    const int lane = tid;
    unsigned long long fl = full[lane];  // word `lane` of the full-class bitmap
    int n_used = state[1];
    bool overflow = false;
    for (int q = 0; q < nq; ++q) {
        // colours of the earlier columns of the round that share a row with q -> extra
        const unsigned long long* cq = cf + (size_t)q * (kRound / 64);
#pragma unroll
        for (int t = 0; t < kRound / 64; ++t) {
            const int p = t * 64 + lane;
            if (p < q && ((cq[t] >> lane) & 1ull)) {
                const int c = col[p];
                atomicOr(&extra[c >> 6], 1ull << (c & 63));
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const unsigned long long taken = F[(size_t)q * kColourWords + lane] | fl | extra[lane];
        extra[lane] = 0ull;
        const unsigned long long fr = ~taken;
        const unsigned long long have = __ballot(fr != 0ull);
        int c;
        if (have == 0ull) {
            overflow = true;
            c = 0;
        } else {
            const int w = __builtin_amdgcn_readfirstlane(__builtin_ctzll(have));  // lowest free word
            const int bit = (fr != 0ull) ? __builtin_ctzll(fr) : 0;
            c = w * 64 + __builtin_amdgcn_readlane(bit, w);
        }
        if (lane == 0) {
            col[q] = c;
            cs[c] += 1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // the class is full once it holds max_batch columns (lane c / 64 keeps that word)
        if (cs[c] >= max_batch && lane == (c >> 6)) fl |= 1ull << (c & 63);
        if (c + 1 > n_used) n_used = c + 1;
    }
    if (overflow && lane == 0) state[0] = 1;
    if (lane == 0) state[1] = n_used;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    for (int x = lane; x < nq; x += 64) {
        colour_out[head + x] = col[x];
        round_colour[x] = col[x];
    }
    for (int x = lane; x < kColourWords * 64; x += 64) class_size[x] = cs[x];
    full[lane] = fl;
}

__global__ __launch_bounds__(256) void colour_commit_kernel(
    int nq, int head, const int32_t* __restrict__ order, const int64_t* __restrict__ cptr,
    const int32_t* __restrict__ cidx, const int64_t* __restrict__ rptr, int32_t* __restrict__ rcnt,
    int32_t* __restrict__ rcol, int32_t* __restrict__ rmcnt,
    const int32_t* __restrict__ round_colour) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    const int32_t j = order[head + q];
    const int32_t c = round_colour[q];
    const int64_t cb = cptr[j], ce = cptr[j + 1];
    for (int64_t ii = cb + threadIdx.x; ii < ce; ii += blockDim.x) {
        const int32_t i = cidx[ii];
        const int32_t slot = atomicAdd(&rcnt[i], 1);
        rcol[rptr[i] + slot] = c;
        rmcnt[i] = 0;  // the next round starts with empty member lists
    }
}

// Device pointers: cptr / cidx (CSC structure), rptr (CSR row pointers of the same matrix).
// order_host: the visiting order.  colour_host[q] = colour of the column at visiting position q.
// Returns hipSuccess with *overflow = 1 when 4096 colours do not suffice (colour_host unspecified).
hipError_t device_first_fit(int64_t n, int32_t d, int64_t nnz, const int64_t* cptr,
                            const int32_t* cidx, const int64_t* rptr, const int32_t* order_host,
                            int max_batch, int32_t* colour_host, int* n_colours, int* overflow,
                            hipStream_t stream) {
    *overflow = 0;
    *n_colours = 0;
    hipError_t e;
    int32_t *d_order = nullptr, *rcnt = nullptr, *rcol = nullptr, *class_size = nullptr,
            *d_colour = nullptr, *round_colour = nullptr, *rmcnt = nullptr, *rmem = nullptr;
    unsigned long long *F = nullptr, *conf = nullptr, *full = nullptr;
    int* state = nullptr;
    auto done = [&](hipError_t rc) {
        (void)hipFree(d_order);
        (void)hipFree(rcnt);
        (void)hipFree(rcol);
        (void)hipFree(rmcnt);
        (void)hipFree(rmem);
        (void)hipFree(class_size);
        (void)hipFree(d_colour);
        (void)hipFree(round_colour);
        (void)hipFree(F);
        (void)hipFree(conf);
        (void)hipFree(full);
        (void)hipFree(state);
        return rc;
    };
    const size_t nz = (size_t)(nnz > 0 ? nnz : 1), nr = (size_t)(n > 0 ? n : 1);
    const size_t conf_words = (size_t)kRound * (kRound / 64);
    if ((e = hipMalloc(&d_order, sizeof(int32_t) * (size_t)d)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&rcnt, sizeof(int32_t) * nr)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&rcol, sizeof(int32_t) * nz)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&rmcnt, sizeof(int32_t) * nr)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&rmem, sizeof(int32_t) * nz)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&class_size, sizeof(int32_t) * kColourWords * 64)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&d_colour, sizeof(int32_t) * (size_t)d)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&round_colour, sizeof(int32_t) * kRound)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&F, sizeof(unsigned long long) * kRound * kColourWords)) != hipSuccess)
        return done(e);
    if ((e = hipMalloc(&conf, sizeof(unsigned long long) * conf_words)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&full, sizeof(unsigned long long) * kColourWords)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&state, sizeof(int) * 2)) != hipSuccess) return done(e);
    if ((e = hipMemcpyAsync(d_order, order_host, sizeof(int32_t) * (size_t)d, hipMemcpyHostToDevice,
                            stream)) != hipSuccess)
        return done(e);
    if ((e = hipMemsetAsync(rcnt, 0, sizeof(int32_t) * nr, stream)) != hipSuccess) return done(e);
    if ((e = hipMemsetAsync(rmcnt, 0, sizeof(int32_t) * nr, stream)) != hipSuccess) return done(e);
    if ((e = hipMemsetAsync(class_size, 0, sizeof(int32_t) * kColourWords * 64, stream)) != hipSuccess)
        return done(e);
    if ((e = hipMemsetAsync(conf, 0, sizeof(unsigned long long) * conf_words, stream)) != hipSuccess)
        return done(e);
    if ((e = hipMemsetAsync(full, 0, sizeof(unsigned long long) * kColourWords, stream)) != hipSuccess)
        return done(e);
    if ((e = hipMemsetAsync(state, 0, sizeof(int) * 2, stream)) != hipSuccess) return done(e);
    const size_t lds = sizeof(unsigned long long) *
                           ((size_t)kRound * kColourWords + conf_words + kColourWords) +
                       sizeof(int) * (kRound + kColourWords * 64);
    if ((e = hipFuncSetAttribute((const void*)colour_resolve_kernel,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess)
        return done(e);
    for (int head = 0; head < d; head += kRound) {
        const int nq = d - head < kRound ? d - head : kRound;
        hipLaunchKernelGGL(colour_snapshot_kernel, dim3(nq), dim3(256), 0, stream, nq, head, d_order,
                           cptr, cidx, rptr, rcnt, rcol, rmcnt, rmem, full, F);
        hipLaunchKernelGGL(colour_conflict_kernel, dim3(nq), dim3(256), 0, stream, nq, head, d_order,
                           cptr, cidx, rptr, rmcnt, rmem, conf);
        hipLaunchKernelGGL(colour_resolve_kernel, dim3(1), dim3(kRound), lds, stream, nq, head,
                           max_batch, F, conf, full, class_size, d_colour, round_colour, state);
        hipLaunchKernelGGL(colour_commit_kernel, dim3(nq), dim3(256), 0, stream, nq, head, d_order,
                           cptr, cidx, rptr, rcnt, rcol, rmcnt, round_colour);
    }
    if ((e = hipGetLastError()) != hipSuccess) return done(e);
    int h_state[2] = {0, 0};
    if ((e = hipMemcpyAsync(h_state, state, sizeof(int) * 2, hipMemcpyDeviceToHost, stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(colour_host, d_colour, sizeof(int32_t) * (size_t)d, hipMemcpyDeviceToHost,
                            stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess)
        return done(e);
    *overflow = h_state[0];
    *n_colours = h_state[1];
    return done(hipSuccess);
}

// ================================================================ RLF colouring (colored_rlf)
// The device form of schedule_rlf (spfm_schedule.cpp, which states the rule): one class at a time
// as a maximal independent set; the first member maximises sum urow over its rows, every later
// one sum wrow, ties to the earliest visiting position.  All keys are integer sums and all
// updates of the row counters are integer adds, so the result is the host's, whatever the
// scheduling.  The work follows a COMPACTED candidate list (positions in the visiting order),
// never d: a member removes its neighbours from the list, which shrinks geometrically.
// One member = three launches, each a wait of the next on the one before (no grid barrier):
//   rlf_key_kernel      one wave per candidate: coalesced over its row indices, gathers the row
//                       counters, integer wave reduction; argmax as atomicMax of
//                       key << 32 | ~position (the larger word = larger key, then earlier position)
//   rlf_pick_kernel     one workgroup: the member's rows get this pick's stamp, urow -= 1; closes
//                       the class at max_batch members or without candidates
//   rlf_exclude_kernel  one wave per candidate: a row with the stamp = a neighbour of the member:
//                       wrow += 1 on all its rows (atomicAdd), else it is appended to the other
//                       candidate buffer (one counter add per 32 candidates)
// The members of a class are queued in chunks without a host round trip; every kernel returns at
// once when the class is closed; the host reads the state words once per chunk.
struct RlfState {
    unsigned long long best;  // argmax word of the pick in flight (0 = none)
    int32_t ncand[2];         // entries of the two candidate buffers
    int32_t closed;           // the class takes no more members
    int32_t class_size;
    int32_t n_done;           // columns coloured so far
    int32_t pick_pos;         // visiting position of the last member
    int32_t fault;            // an index out of range was seen (never expected)
    int32_t pad;
};

constexpr int kRlfChunk = 32;       // candidates per workgroup iteration (4 waves x 8)
constexpr int kRlfMaxBlocks = 2048;
constexpr int kRlfQueue = 32;       // members queued between two reads of the state

__global__ __launch_bounds__(256) void rlf_urow_kernel(int64_t n, const int64_t* __restrict__ rptr,
                                                       int32_t* __restrict__ urow) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) urow[i] = (int32_t)(rptr[i + 1] - rptr[i]);
}

// candidates of a new class: the uncoloured positions (any order: the argmax word carries the
// position)
__global__ __launch_bounds__(256) void rlf_begin_kernel(int32_t d, const uint8_t* __restrict__ coloured,
                                                        int32_t* __restrict__ cand,
                                                        RlfState* __restrict__ st) {
    __shared__ int32_t base;
    __shared__ int32_t wcount[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int32_t p0 = blockIdx.x * 256; p0 < d; p0 += gridDim.x * 256) {
        const int32_t pos = p0 + (int32_t)threadIdx.x;
        const bool keep = pos < d && !coloured[pos];
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0)
            base = atomicAdd(&st->ncand[0], wcount[0] + wcount[1] + wcount[2] + wcount[3]);
        __syncthreads();
        if (keep) {
            int32_t at = base + __popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) at += wcount[w];
            cand[at] = pos;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rlf_key_kernel(
    int cur, const int32_t* __restrict__ cand, const int32_t* __restrict__ order,
    const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx,
    const int32_t* __restrict__ cnt, RlfState* __restrict__ st) {
    if (st->closed) return;
    __shared__ unsigned long long wbest[4];
    const int32_t nc = st->ncand[cur];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long best = 0ull;
    for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < nc; c += (int64_t)gridDim.x * 4) {
        const int32_t pos = cand[c];
        const int32_t j = order[pos];
        const int64_t cb = cptr[j], ce = cptr[j + 1];
        unsigned int key = 0;
        for (int64_t ii = cb + lane; ii < ce; ii += 64) key += (unsigned int)cnt[cidx[ii]];
        for (int off = 32; off > 0; off >>= 1) key += __shfl_xor(key, off);
        const unsigned long long w =
            ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)pos);
        best = w > best ? w : best;
    }
    if (lane == 0) wbest[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = wbest[w] > best ? wbest[w] : best;
        if (best) atomicMax(&st->best, best);
    }
}

__global__ __launch_bounds__(256) void rlf_pick_kernel(
    int cur, int32_t d, int64_t n, int32_t stamp, int max_batch, const int32_t* __restrict__ order,
    const int64_t* __restrict__ cptr, const int32_t* __restrict__ cidx, int32_t* __restrict__ urow,
    int32_t* __restrict__ mark, uint8_t* __restrict__ coloured, int32_t* __restrict__ out_pos,
    RlfState* __restrict__ st) {
    if (st->closed) return;
    const unsigned long long best = st->best;
    const int32_t nc = st->ncand[cur];
    const int32_t n_done = st->n_done, csize = st->class_size;
    __syncthreads();  // every thread has read the state before thread 0 rewrites it
    const unsigned int pos = 0xFFFFFFFFu - (unsigned int)(best & 0xFFFFFFFFull);
    if (nc <= 0 || best == 0ull || pos >= (unsigned int)d || n_done >= d) {
        if (threadIdx.x == 0) {
            st->closed = 1;
            if (nc > 0) st->fault = 1;
        }
        return;
    }
    const int32_t j = order[pos];
    const int64_t cb = cptr[j], ce = cptr[j + 1];
    for (int64_t ii = cb + threadIdx.x; ii < ce; ii += blockDim.x) {
        const int32_t i = cidx[ii];
        if (i < 0 || i >= n) continue;
        mark[i] = stamp;
        urow[i] -= 1;  // the rows of one column are distinct
    }
    if (threadIdx.x == 0) {
        coloured[pos] = 1;
        out_pos[n_done] = (int32_t)pos;
        st->n_done = n_done + 1;
        st->class_size = csize + 1;
        st->pick_pos = (int32_t)pos;
        st->best = 0ull;
        st->ncand[1 - cur] = 0;
        if (csize + 1 >= max_batch) st->closed = 1;
    }
}

__global__ __launch_bounds__(256) void rlf_exclude_kernel(
    int cur, int32_t stamp, const int32_t* __restrict__ cand_in, int32_t* __restrict__ cand_out,
    const int32_t* __restrict__ order, const int64_t* __restrict__ cptr,
    const int32_t* __restrict__ cidx, const int32_t* __restrict__ mark, int32_t* __restrict__ wrow,
    RlfState* __restrict__ st) {
    if (st->closed) return;
    __shared__ int32_t keep_pos[kRlfChunk];
    const int32_t nc = st->ncand[cur];
    const int32_t picked = st->pick_pos;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c0 = (int64_t)blockIdx.x * kRlfChunk; c0 < nc; c0 += (int64_t)gridDim.x * kRlfChunk) {
        for (int t = 0; t < kRlfChunk / 4; ++t) {
            const int slot = t * 4 + wave;
            const int64_t c = c0 + slot;
            int32_t keep = -1;
            if (c < nc) {
                const int32_t pos = cand_in[c];
                if (pos != picked) {
                    const int32_t j = order[pos];
                    const int64_t cb = cptr[j], ce = cptr[j + 1];
                    bool hit = false;
                    for (int64_t ii = cb + lane; ii < ce; ii += 64) hit |= mark[cidx[ii]] == stamp;
                    if (__ballot(hit) != 0ull) {
                        for (int64_t ii = cb + lane; ii < ce; ii += 64) atomicAdd(&wrow[cidx[ii]], 1);
                    } else {
                        keep = pos;
                    }
                }
            }
            if (lane == 0) keep_pos[slot] = keep;
        }
        __syncthreads();
        if (wave == 0) {
            const int32_t p = lane < kRlfChunk ? keep_pos[lane] : -1;
            const unsigned long long m = __ballot(p >= 0);
            int32_t base = 0;
            if (lane == 0 && m) base = atomicAdd(&st->ncand[1 - cur], __popcll(m));
            base = __shfl(base, 0);
            if (p >= 0) cand_out[base + __popcll(m & ((1ull << lane) - 1ull))] = p;
        }
        __syncthreads();
    }
}

// Device pointers: cptr / cidx (CSC structure), rptr (CSR row pointers of the same matrix).
// order_host: the visiting order.  Fills out_order (classes concatenated, their columns in visiting
// order) and batch_ptr.  *failed = 1 (and hipSuccess) when the device state was inconsistent:
// like any error, the host form takes over.
hipError_t device_rlf(int64_t n, int32_t d, int64_t nnz, const int64_t* cptr, const int32_t* cidx,
                      const int64_t* rptr, const int32_t* order_host, int max_batch,
                      std::vector<int32_t>& out_order, std::vector<int32_t>& batch_ptr, int* failed,
                      hipStream_t stream) {
    *failed = 0;
    hipError_t e;
    int32_t *d_order = nullptr, *urow = nullptr, *wrow = nullptr, *mark = nullptr, *cand0 = nullptr,
            *cand1 = nullptr, *out_pos = nullptr;
    uint8_t* coloured = nullptr;
    RlfState* st = nullptr;
    auto done = [&](hipError_t rc) {
        (void)hipFree(d_order);
        (void)hipFree(urow);
        (void)hipFree(wrow);
        (void)hipFree(mark);
        (void)hipFree(cand0);
        (void)hipFree(cand1);
        (void)hipFree(out_pos);
        (void)hipFree(coloured);
        (void)hipFree(st);
        return rc;
    };
    (void)nnz;
    const size_t nr = (size_t)(n > 0 ? n : 1), nd = (size_t)d;
    if ((e = hipMalloc(&d_order, sizeof(int32_t) * nd)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&urow, sizeof(int32_t) * nr)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&wrow, sizeof(int32_t) * nr)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&mark, sizeof(int32_t) * nr)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&cand0, sizeof(int32_t) * nd)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&cand1, sizeof(int32_t) * nd)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&out_pos, sizeof(int32_t) * nd)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&coloured, nd)) != hipSuccess) return done(e);
    if ((e = hipMalloc(&st, sizeof(RlfState))) != hipSuccess) return done(e);
    if ((e = hipMemcpyAsync(d_order, order_host, sizeof(int32_t) * nd, hipMemcpyHostToDevice,
                            stream)) != hipSuccess)
        return done(e);
    if ((e = hipMemsetAsync(mark, 0, sizeof(int32_t) * nr, stream)) != hipSuccess) return done(e);
    if ((e = hipMemsetAsync(urow, 0, sizeof(int32_t) * nr, stream)) != hipSuccess) return done(e);
    if ((e = hipMemsetAsync(coloured, 0, nd, stream)) != hipSuccess) return done(e);
    if ((e = hipMemsetAsync(st, 0, sizeof(RlfState), stream)) != hipSuccess) return done(e);
    if (n > 0)
        hipLaunchKernelGGL(rlf_urow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n,
                           rptr, urow);
    int32_t* cand[2] = {cand0, cand1};
    std::vector<int32_t> bp(1, 0);
    int32_t n_done = 0, stamp = 0;
    int last_size = kRlfQueue;
    RlfState hs;
    while (n_done < d) {
        // a new class: wrow = 0, the state words of the class = 0, cand[0] = the uncoloured positions
        const int32_t left = d - n_done;
        if ((e = hipMemsetAsync(wrow, 0, sizeof(int32_t) * nr, stream)) != hipSuccess) return done(e);
        if ((e = hipMemsetAsync(st, 0, offsetof(RlfState, n_done), stream)) != hipSuccess)
            return done(e);
        hipLaunchKernelGGL(rlf_begin_kernel, dim3((unsigned)std::min(kRlfMaxBlocks, (d + 255) / 256)),
                           dim3(256), 0, stream, d, coloured, cand0, st);
        const unsigned kb = (unsigned)std::min(kRlfMaxBlocks, (left + 3) / 4);
        const unsigned xb = (unsigned)std::min(kRlfMaxBlocks, (left + kRlfChunk - 1) / kRlfChunk);
        int picks = 0;
        bool closed = false;
        // (the first queue of a class is as long as the last class was, plus a few: a matrix
        // whose classes are tiny does not pay for launches that only find the class closed)
        int queue = std::min(kRlfQueue, std::max(4, last_size + 4));
        while (!closed) {
            for (int t = 0; t < queue && picks < max_batch; ++t, ++picks) {
                const int cur = picks & 1;
                ++stamp;
                hipLaunchKernelGGL(rlf_key_kernel, dim3(kb), dim3(256), 0, stream, cur, cand[cur],
                                   d_order, cptr, cidx, picks == 0 ? urow : wrow, st);
                hipLaunchKernelGGL(rlf_pick_kernel, dim3(1), dim3(256), 0, stream, cur, d, n, stamp,
                                   max_batch, d_order, cptr, cidx, urow, mark, coloured, out_pos, st);
                hipLaunchKernelGGL(rlf_exclude_kernel, dim3(xb), dim3(256), 0, stream, cur, stamp,
                                   cand[cur], cand[1 - cur], d_order, cptr, cidx, mark, wrow, st);
            }
            if ((e = hipGetLastError()) != hipSuccess) return done(e);
            if ((e = hipMemcpyAsync(&hs, st, sizeof(RlfState), hipMemcpyDeviceToHost, stream)) !=
                    hipSuccess ||
                (e = hipStreamSynchronize(stream)) != hipSuccess)
                return done(e);
            // (after `picks` members the live candidates are in buffer picks & 1)
            closed = hs.closed || picks >= max_batch || hs.ncand[picks & 1] == 0;
            queue = kRlfQueue;
            if (hs.fault || hs.n_done != n_done + hs.class_size || hs.class_size > picks) {
                *failed = 1;
                return done(hipSuccess);
            }
        }
        if (hs.class_size <= 0) {  // no progress: cannot happen while columns are left
            *failed = 1;
            return done(hipSuccess);
        }
        n_done = hs.n_done;
        last_size = hs.class_size;
        bp.push_back(n_done);
    }
    std::vector<int32_t> pos((size_t)d);
    if ((e = hipMemcpyAsync(pos.data(), out_pos, sizeof(int32_t) * nd, hipMemcpyDeviceToHost,
                            stream)) != hipSuccess ||
        (e = hipStreamSynchronize(stream)) != hipSuccess)
        return done(e);
    out_order.assign((size_t)d, 0);
    for (size_t b = 0; b + 1 < bp.size(); ++b) {
        std::sort(pos.begin() + bp[b], pos.begin() + bp[b + 1]);
        for (int32_t q = bp[b]; q < bp[b + 1]; ++q) out_order[(size_t)q] = order_host[pos[(size_t)q]];
    }
    batch_ptr = std::move(bp);
    return done(hipSuccess);
}

}  // namespace spfm
