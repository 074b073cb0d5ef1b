"""What a weighted fit costs per iteration, on one MI355X.

Two coordinate-descent lines -- the config-2 shape (pcd, squaredl12, degree 2, k = 30) and the
config-4 shape (pbcd, omegacs, degree 2, k = 30) of bench.py, scaled to 100k x 10k at 50 nnz per
row, coloured schedule, f32 -- each timed three ways on three handles that share ONE device image:

  (a) unweighted as shipped        the persistent pass
  (b) unweighted, multi-kernel     options persistent = 0 / pbcd_persistent = 0
  (c) weighted                     weights uniform in [0.5, 1.5]; runs on the engine of (b)

(c) against (b) is the price of the weight gather (one f64 per entry of a column); (c) against (a)
is the price of leaving the persistent pass.  One psgd line on the shape of tools/bench_psgd.py
(1M x 100k, k = 30, l1, batch_size = 1 / density): unweighted against weighted epochs.

An iteration is bench.py's: cd_linear, then the pcd (all components) or pbcd epoch.  Host clock
around calls that end in a device synchronise; after one warm-up iteration of each handle the
handles alternate, medians of --repeats.  Writes profiles/weights_<build tag>.json unless --out is
given.  Nothing is asserted.

    python tools/bench_weighted.py [--rows 100000] [--cols 10000] [--repeats 5] [--skip-psgd]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NNZ_PER_ROW = 50
CONFIGS = {  # bench.py CONFIGS[2] and [4]
    2: dict(solver="pcd", reg="squaredl12", degree=2, k=30, alpha=1.0, beta=10.0, gamma=1e-4),
    4: dict(solver="pbcd", reg="omegacs", degree=2, k=30, alpha=1.0, beta=1.0, gamma=1e-3),
}


def _stats(ts):
    ts = np.array(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(ts.min()), 3),
                max_ms=round(float(ts.max()), 3), all_ms=[round(float(t), 3) for t in ts])


def _iteration(eng, cfg):
    ic = np.arange(cfg["k"], dtype=np.int32)
    v = eng.cd_linear_epoch(cfg["alpha"])
    if cfg["solver"] == "pcd":
        return v + eng.pcd_epoch(0, 2, cfg["beta"], cfg["gamma"], 1.0, ic)
    return v + eng.pbcd_epoch(0, 2, cfg["beta"], cfg["gamma"], 1.0)


def _alternate(run, names, warmup, repeats):
    times = {m: [] for m in names}
    for rep in range(warmup + repeats):
        for m in names:
            t0 = time.perf_counter()
            run(m)
            if rep >= warmup:
                times[m].append(time.perf_counter() - t0)
    return times


def cd_line(cfg_id, n, d, weights, a):
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.synth import make_problem

    cfg = CONFIGS[cfg_id]
    X, y = make_problem(n, d, NNZ_PER_ROW, seed=0)
    Xc = X.tocsc()
    Xc.sort_indices()
    P0 = 0.01 * np.random.RandomState(0).randn(1, cfg["k"], d)
    engs, active = {}, {}
    for name in ("unweighted", "unweighted_multi_kernel", "weighted"):
        eng = HipEngine(0, "f32")
        if name != "unweighted":
            eng.set_option("persistent", 0)
            eng.set_option("pbcd_persistent", 0)
        if engs:
            eng.share_data(engs["unweighted"])
        else:
            eng.set_data(Xc, y)
        if name == "weighted":
            eng.set_sample_weight(weights)
        eng.set_params(P0, np.zeros(d), np.ones(cfg["k"]))
        eng.configure(cfg["solver"], "squared", cfg["reg"], 2)
        eng.init_pred(2, True, False)
        eng.set_schedule("colored", np.arange(d, dtype=np.int32))
        engs[name] = eng
    times = _alternate(lambda m: _iteration(engs[m], cfg), list(engs), a.warmup, a.repeats)
    for name, eng in engs.items():
        active[name] = dict(persistent_active=eng.get_option("persistent_active"),
                            pbprb_active=eng.get_option("pbprb_active"))
    line = dict(config=cfg_id, solver=cfg["solver"], regularizer=cfg["reg"], k=cfg["k"], n=n, d=d,
                nnz=int(Xc.nnz), dependent_steps_per_sweep=engs["weighted"].n_batches,
                engines=active, **{m: _stats(t) for m, t in times.items()})
    med = {m: line[m]["median_ms"] for m in times}
    line["weighted_over_multi_kernel"] = round(med["weighted"] / med["unweighted_multi_kernel"], 4)
    line["weighted_over_unweighted"] = round(med["weighted"] / med["unweighted"], 4)
    for eng in engs.values():
        eng.close()
    return line


def psgd_line(a):
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.synth import make_problem

    n, d, k = a.psgd_rows, a.psgd_cols, 30
    X, y = make_problem(n, d, NNZ_PER_ROW, 0)
    Xc = X.tocsc()
    Xc.sort_indices()
    batch = int(n * d / Xc.nnz)
    weights = np.random.RandomState(1).uniform(0.5, 1.5, size=n)
    idx = np.arange(n, dtype=np.int32)
    args = (2, 1e-3, 1e-3, 1e-3, 0.01, "optimal", 1.0, batch, idx, True)
    engs, its = {}, {}
    for name in ("unweighted", "weighted"):
        eng = HipEngine(0, "f32")
        if engs:
            eng.share_data(engs["unweighted"])
            eng.set_sample_weight(weights)
        else:
            eng.set_data(Xc, y)
        eng.set_params(0.01 * np.random.RandomState(0).randn(1, k, d), np.zeros(d), np.ones(k))
        eng.configure("psgd", "squared", "l1", 2)
        engs[name], its[name] = eng, 1

    def run(m):
        _, its[m] = engs[m].psgd_epoch(*args, its[m])

    times = _alternate(run, list(engs), a.warmup, a.repeats)
    line = dict(solver="psgd", regularizer="l1", k=k, n=n, d=d, nnz=int(Xc.nnz), batch_size=batch,
                updates_per_epoch=-(-n // batch), **{m: _stats(t) for m, t in times.items()})
    line["weighted_over_unweighted"] = round(line["weighted"]["median_ms"]
                                             / line["unweighted"]["median_ms"], 4)
    for eng in engs.values():
        eng.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--cols", type=int, default=10_000)
    ap.add_argument("--psgd-rows", type=int, default=1_000_000)
    ap.add_argument("--psgd-cols", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-psgd", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f32")
    res = dict(tool="bench_weighted", build_tag=_capi.build_tag(), device_name=eng.device_name,
               precision="f32", schedule="colored", warmup=a.warmup, repeats=a.repeats,
               timing="host clock around an iteration that ends in a device synchronise; the "
                      "handles of a line share one device image and alternate",
               lines=[])
    eng.close()
    weights = np.random.RandomState(1).uniform(0.5, 1.5, size=a.rows)
    for cfg_id in (2, 4):
        line = cd_line(cfg_id, a.rows, a.cols, weights, a)
        res["lines"].append(line)
        print(json.dumps(line), flush=True)
    if not a.skip_psgd:
        line = psgd_line(a)
        res["lines"].append(line)
        print(json.dumps(line), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "weights_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
