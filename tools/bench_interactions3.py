"""Third-order interaction weights on the device against the host einsum.

k = 30 components, d_a in {1 000, 4 000, 10 000} active features (all columns non-zero),
parameters only (no data set is needed):

  (a) device:  interaction3_stats and interaction3_topk(1000) of sparsepoly_amd.engine.HipEngine
  (b) host:    numpy.einsum('s,sa,sj,sl->ajl', lams, P, P, P, optimize=True) and a count of its
               non-zeros, at the largest d_a whose d_a^3 doubles fit --host-bytes (the tensor the
               device never stores), on 16 threads

Warm-up, repeats, median and spread of each; flops per pass (d_a^3 k / 3), the rate they imply,
the scratch the entries hold and the library's build tag go into the output.  Writes
profiles/interactions3_<build tag>.json unless --out is given.  Nothing is asserted.

    python tools/bench_interactions3.py [--features 1000,4000,10000] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                repeats=int(repeats))


def _host(P, lams):
    T = np.einsum("s,sa,sj,sl->ajl", lams, P, P, P, optimize=True)
    return int(np.count_nonzero(T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="1000,4000,10000")
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--topk", type=int, default=1000)
    ap.add_argument("--host-bytes", type=float, default=4e9,
                    help="the host einsum runs at the largest d_a with 8 d_a^3 below this")
    ap.add_argument("--host-features", default="100,200,400,800",
                    help="candidate sizes for the host einsum")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    k = a.components
    rng = np.random.RandomState(0)
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    eng = HipEngine(0, "f32")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name,
               shape=dict(components=k, topk=a.topk), cases=[])
    for da in [int(f) for f in a.features.split(",")]:
        P = 0.1 * rng.randn(k, da)
        eng.set_params(P[None], np.zeros(da), lams)
        st = eng.interaction3_stats(0)
        flops = da ** 3 * k / 3.0
        case = dict(active_features=st["active_features"], triples=da * (da - 1) * (da - 2) // 6,
                    nnz=st["nnz"], flops_per_pass=flops,
                    stats=_timed(lambda: eng.interaction3_stats(0), a.warmup, a.repeats),
                    stats_launches=eng.get_option("interaction_launches"),
                    topk=_timed(lambda: eng.interaction3_topk(0, a.topk), a.warmup, a.repeats),
                    scratch_kib=eng.get_option("interaction_scratch_kib"))
        case["stats_tflops"] = flops / (case["stats"]["median_ms"] * 1e-3) / 1e12
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    eng.close()
    fits = [int(f) for f in a.host_features.split(",") if 8.0 * int(f) ** 3 <= a.host_bytes]
    if fits:
        dh = max(fits)
        P = 0.1 * rng.randn(k, dh)
        host = _timed(lambda: _host(P, lams), 0, max(1, min(a.repeats, 3)))
        host.update(features=dh, tensor_bytes=8.0 * dh ** 3)
        res["host_einsum"] = host
        print(json.dumps(host), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "interactions3_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
