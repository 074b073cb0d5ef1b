"""Selected interactions on the device against the dense host recipe.

Config-2 parameter shape (k = 30, d = 100 000) at three active fractions (1 %, 10 %, 100 % of the
columns non-zero), parameters only (no data set is needed):

  (a) device:  interaction_stats and interaction_topk(1000) of sparsepoly_amd.engine.HipEngine
  (b) host:    P_a.T @ (lams[:, None] * P_a) on the active columns, count_nonzero of the upper
               triangle, argpartition for the top 1000 -- what the reference's example does, on
               16 threads.  Where the d_a x d_a product does not fit the host budget it runs on
               a 20 000-feature slice and its time is scaled by the pair count (marked "scaled").

Warm-up, repeats, median and spread of each; the library's build tag goes into the output.
Writes profiles/interactions_<build tag>.json unless --out is given.  Nothing is asserted.

    python tools/bench_interactions.py [--features 100000] [--repeats 5] [--out FILE]
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


def _host(Pa, lams, K):
    W = Pa.T @ (lams[:, None] * Pa)
    iu = np.triu_indices(W.shape[0], k=1)
    we = W[iu]
    nnz = int(np.count_nonzero(we))
    top = np.argpartition(-np.abs(we), min(K, we.size - 1))[:K]
    return nnz, top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--fractions", default="0.01,0.1,1.0")
    ap.add_argument("--topk", type=int, default=1000)
    ap.add_argument("--host-slice", type=int, default=20_000)
    ap.add_argument("--host-max-features", type=int, default=20_000,
                    help="largest d_a whose dense product the host baseline forms whole")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    d, k = a.features, a.components
    rng = np.random.RandomState(0)
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    eng = HipEngine(0, "f32")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name,
               shape=dict(features=d, components=k, topk=a.topk), cases=[])
    for frac in [float(f) for f in a.fractions.split(",")]:
        P = 0.1 * rng.randn(k, d)
        P[:, rng.rand(d) >= frac] = 0.0
        active = np.flatnonzero((P != 0).any(axis=0))
        da = len(active)
        eng.set_params(P[None], np.zeros(d), lams)
        st = eng.interaction_stats(0)
        case = dict(active_fraction=frac, active_features=da, pairs=da * (da - 1) // 2,
                    nnz=st["nnz"], flops_per_pass=2.0 * da * da / 2 * k,
                    stats=_timed(lambda: eng.interaction_stats(0), a.warmup, a.repeats),
                    topk=_timed(lambda: eng.interaction_topk(0, a.topk), a.warmup, a.repeats),
                    scratch_kib=eng.get_option("interaction_scratch_kib"))
        dh = min(da, a.host_slice if da > a.host_max_features else da)
        Pa = np.ascontiguousarray(P[:, active[:dh]])
        host = _timed(lambda: _host(Pa, lams, a.topk), 0, max(1, min(a.repeats, 3)))
        scale = (da * (da - 1.0)) / (dh * (dh - 1.0)) if dh > 1 else 1.0
        host.update(scaled=bool(dh < da), slice_features=dh, scale=scale,
                    median_ms_full=host["median_ms"] * scale)
        case["host"] = host
        case["ratio_host_over_device"] = host["median_ms_full"] / (
            case["stats"]["median_ms"] + case["topk"]["median_ms"])
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    eng.close()
    out = a.out or os.path.join(ROOT, "profiles", "interactions_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
