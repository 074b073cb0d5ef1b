"""Objective terms + held-out loss of a live fit: the device path against what a callback has to
do without it.

Config-2 matrix (sparsepoly_amd.synth: 1M x 100k, ~50 nnz per row, k = 30, degree 2, pcd +
squaredl12), one coloured iteration, then

  (a) device:   objective_terms of every block and of w, loss_sum, eval_loss on a resident
                100k-row held-out set
  (b) callback: get_params, host regularizer.eval + NumPy for the same numbers, predict on the
                held-out set through a fresh engine (parameter and matrix upload per call)

Warm-up, repeats, median and spread of each; the library's build tag goes into the output.
Writes profiles/objective_<build tag>.json unless --out is given.  Nothing is asserted.

    python tools/bench_objective.py [--rows 1000000] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--val-rows", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.regularizer import SquaredL12
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(a.rows, a.features, seed=0)
    Xv, yv = make_problem(a.val_rows, a.features, seed=1)
    d, k = a.features, a.components
    eng = HipEngine(0, "f32")
    eng.set_data(X, y)
    eng.set_params(0.01 * np.random.RandomState(0).randn(1, k, d), np.zeros(d), np.ones(k))
    eng.configure("pcd", "squared", "squaredl12", 2)
    eng.init_pred(2, True, False)
    eng.set_schedule("colored", np.arange(d, dtype=np.int32))
    eng.cd_linear_epoch(1e-3)
    eng.pcd_epoch(0, 2, 1e-3, 1e-5, 1.0, np.arange(k, dtype=np.int32))
    eng.set_eval_data(Xv, yv)

    def device():
        t = eng.objective_terms(0, 2)
        tw = eng.objective_terms(-1, 1)
        return eng.loss_sum(), t, tw, eng.eval_loss(2, True, False)

    reg = SquaredL12()

    def callback():
        P, w = eng.get_params()
        omega = reg.eval(P[0].T, 2)
        l2 = 0.5 * float((P[0] * P[0]).sum())
        nz = P[0] != 0
        counts = (int(nz.sum()), int(nz.any(axis=0).sum()), int(nz.any(axis=1).sum()))
        fresh = HipEngine(0, "f32")
        try:
            fresh.set_params(P, w, np.ones(k))
            pred = fresh.predict(Xv, 2, True, False)
        finally:
            fresh.close()
        return eng.loss_sum(), omega, l2, counts, 0.5 * float(((pred - yv) ** 2).sum())

    dv, cb = device(), callback()
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name,
               shape=dict(rows=a.rows, features=d, components=k, val_rows=a.val_rows),
               values=dict(device_omega=dv[1]["omega"], host_omega=float(cb[1]),
                           device_val_loss=dv[3], host_val_loss=cb[4]),
               device=_timed(device, a.warmup, a.repeats),
               callback=_timed(callback, a.warmup, a.repeats))
    res["ratio_callback_over_device"] = res["callback"]["median_ms"] / res["device"]["median_ms"]
    eng.close()
    out = a.out or os.path.join(ROOT, "profiles", "objective_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
