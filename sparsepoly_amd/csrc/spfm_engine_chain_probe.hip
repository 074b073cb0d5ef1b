// spfm_engine_chain_probe.hip -- spfm_debug_chain: the production chains of the pcd passes
// (pcd_chain_lanes, pcd_chain_waves; spfm_pcd.hip.h) run on given column values, for the tests
// that pin them column by column (tests/test_hip_chain.py).  Nothing here is on a hot path.
#include "spfm_engine.hip.h"
#include "spfm_pcd.hip.h"

using namespace spfm;

namespace {

// in: [3][ncols] = p_old, g, hsum; out: [ncols] new coordinates, then the M + 1 cache values
struct ChainProbeArgs {
    int reg, ncols;
    const double* in;
    const double* cache_in;
    double* out;
    double lam, mu, beta, gamma, eta;
};

// one wave, called as the control wave of pcd_prb_kernel calls the chain
template <int M>
__global__ __launch_bounds__(kWave) void chain_probe_lanes_kernel(ChainProbeArgs a) {
    __shared__ double sh_chain[(kWave + 4) * 4];
    const int lane = threadIdx.x;
    const bool valid = lane < a.ncols;
    double cache[M + 1];
#pragma unroll
    for (int t = 0; t <= M; ++t) cache[t] = a.cache_in[t];
    const double pl = valid ? a.in[lane] : 0.0;
    const double g = valid ? a.in[a.ncols + lane] : 0.0;
    const double hs = valid ? a.in[2 * a.ncols + lane] : 0.0;
    const double res = pcd_chain_lanes<M>(a.reg, lane, a.ncols - 1, valid, pl, g, hs, a.lam, a.mu,
                                          a.beta, a.gamma, a.eta, cache, sh_chain);
    if (valid) a.out[lane] = res;
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t <= M; ++t) a.out[a.ncols + t] = cache[t];
    }
}

// one workgroup of eight waves, called as pcdw_kernel calls the wide chain
__global__ __launch_bounds__(512) void chain_probe_waves_kernel(ChainProbeArgs a) {
    __shared__ double sh_map[16];
    __shared__ int sh_bad[3];
    const int q = threadIdx.x;
    const int wave = q >> 6, wlane = q & 63;
    const bool valid = q < a.ncols;
    double cache[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) cache[t] = a.cache_in[t];
    const double s0 = valid ? a.in[q] : 0.0;
    const double t0 = valid ? a.in[a.ncols + q] : 0.0;
    const double t1 = valid ? a.in[2 * a.ncols + q] : 0.0;
    const double res = pcd_chain_waves<2>(a.reg, wlane, wave, a.ncols, valid, s0, t0, t1, a.lam, a.mu,
                                          a.beta, a.gamma, a.eta, cache, sh_map, sh_bad);
    if (valid) a.out[q] = res;
    if (q == 0) {
#pragma unroll
        for (int t = 0; t < 3; ++t) a.out[a.ncols + t] = cache[t];
    }
}

}  // namespace

SPFM_DEFINE_BRANCH_COUNTS(spfm_branch_counts_chain_probe)

extern "C" int spfm_debug_chain(spfm_handle h, int form, int reg, int degree, int ncols,
                                const double* p_old, const double* g, const double* hsum,
                                double lam, double mu, double beta, double gamma, double eta,
                                const double* cache_in, double* p_new, double* cache_out) {
    SPFM_GUARD(h);
    if ((form != 0 && form != 1) || !p_old || !g || !hsum || !cache_in || !p_new || !cache_out)
        return SPFM_ERR_INVALID;
    if (reg != REG_L1 && reg != REG_SQL12 && reg != REG_OMEGATI) return SPFM_ERR_INVALID;
    if (degree != 0 && (degree < 2 || degree > kMaxDegree)) return SPFM_ERR_INVALID;
    if (reg == REG_SQL12 && degree != 2) return SPFM_ERR_INVALID;  // squaredl12.py: degree 2 only
    if (form == 1 && degree != 2) return SPFM_ERR_INVALID;         // wide steps: degree 2
    if (ncols < 1 || ncols > (form == 0 ? kWave : 8 * kWave)) return SPFM_ERR_INVALID;
    const int nc = degree + 1;  // cache values (all-subsets: the running product alone)
    std::vector<double> host((size_t)3 * ncols + nc);
    memcpy(host.data(), p_old, sizeof(double) * ncols);
    memcpy(host.data() + ncols, g, sizeof(double) * ncols);
    memcpy(host.data() + 2 * (size_t)ncols, hsum, sizeof(double) * ncols);
    memcpy(host.data() + 3 * (size_t)ncols, cache_in, sizeof(double) * nc);
    DevBuf din, dout;
    if (din.alloc(sizeof(double) * host.size()) != hipSuccess ||
        dout.alloc(sizeof(double) * ((size_t)ncols + nc)) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    if (hipMemcpyAsync(din.p, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice,
                       h->stream) != hipSuccess)
        return SPFM_ERR_RUNTIME;
    ChainProbeArgs a{};
    a.reg = reg;
    a.ncols = ncols;
    a.in = din.as<double>();
    a.cache_in = din.as<double>() + 3 * (size_t)ncols;
    a.out = dout.as<double>();
    a.lam = lam;
    a.mu = mu;
    a.beta = beta;
    a.gamma = gamma;
    a.eta = eta;
    if (form == 1) {
        hipLaunchKernelGGL(chain_probe_waves_kernel, dim3(1), dim3(512), 0, h->stream, a);
    } else {
        SPFM_DISPATCH_KIND(degree, true,
                           hipLaunchKernelGGL(chain_probe_lanes_kernel<M>, dim3(1), dim3(kWave), 0,
                                              h->stream, a));
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) {
        h->err = "chain probe kernel failed";
        return SPFM_ERR_RUNTIME;
    }
    std::vector<double> res((size_t)ncols + nc);
    if (hipMemcpy(res.data(), dout.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost) !=
        hipSuccess)
        return SPFM_ERR_RUNTIME;
    memcpy(p_new, res.data(), sizeof(double) * ncols);
    memcpy(cache_out, res.data() + ncols, sizeof(double) * nc);
    return SPFM_OK;
}
