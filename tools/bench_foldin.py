"""Fold-in of new user columns on the device against the host recipe on the same inputs.

Synthetic shape: --columns (10 000) new one-hot user columns, --rows-per-column (20) rows each,
every row --row-nnz (30) stored entries: the new user's 1 and 29 entries over --features (100 000)
trained columns; k = --components (30).  Two lines: degree 2 with squared loss (R = 31 unknowns
per column) and degree 3 'explicit' with logistic loss (two blocks, R = 61).  Per line, medians of
--repeats after --warmup calls on one GPU, f64 handle:

  (a) fold_in:  est.fold_in(X, y, columns) -- the device time of its kernels (spfm_foldin_info:
                the design kernel per block and the solve; not the copies) and the wall time of
                the whole call (checks, row gather, copies, handle)
  (b) host:     restate_fold_in(..., n_threads=--threads (16)) in float64 on the same inputs, the
                point of comparison: the NumPy design and one Newton iteration per column

and the ratio host wall / fold_in wall, the one claim to make.  Writes
profiles/foldin_<build tag>.json unless --out is given.  Nothing is asserted.

    python tools/bench_foldin.py [--columns 10000] [--repeats 5] [--host-repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median(ts):
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                repeats=int(len(ts)))


def _estimator(degree, loss, a, d):
    from sklearn.preprocessing import LabelBinarizer
    from sparsepoly_amd import (SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)

    rng = np.random.RandomState(degree)
    k = a.components
    if loss == "squared":
        est = SparseFactorizationMachineRegressor(degree=degree, n_components=k, precision="f64",
                                                  alpha=1.0, beta=1.0, device=0)
    else:
        est = SparseFactorizationMachineClassifier(degree=degree, loss=loss, n_components=k,
                                                   precision="f64", alpha=1.0, beta=1.0, device=0)
        est.label_binarizer_ = LabelBinarizer(pos_label=1, neg_label=-1).fit([-1, 1])
    est.P_ = 0.1 * rng.randn(degree - 1, k, d)
    est.w_ = 0.1 * rng.randn(d)
    est.lams_ = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    return est


def _line(degree, loss, X, cols, a):
    from sparsepoly_amd.foldin import restate_fold_in

    est = _estimator(degree, loss, a, X.shape[1])
    rng = np.random.RandomState(100 + degree)
    y = rng.randn(X.shape[0]) if loss == "squared" else np.where(rng.rand(X.shape[0]) < 0.5, -1., 1.)
    dev, wall, res = [], [], None
    for rep in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        res = est.fold_in(X, y, cols)
        t1 = time.perf_counter()
        if rep >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(res.info["device_ms"])
    host, ref = [], None
    for rep in range(a.host_repeats):
        t0 = time.perf_counter()
        ref = restate_fold_in(est, X, y, cols, n_threads=a.threads)
        host.append((time.perf_counter() - t0) * 1e3)
    line = dict(degree=degree, loss=loss, components=a.components, columns=int(len(cols)),
                rows=int(X.shape[0]), row_nnz=a.row_nnz, unknowns=int(res.theta.shape[1]),
                fold_in=dict(device=_median(dev), wall=_median(wall), groups=res.info["groups"],
                             scratch_kib=res.info["scratch_kib"]),
                host=dict(wall=_median(host), threads=a.threads),
                converged=int(res.converged.sum()), iterations_max=int(res.n_iter.max()),
                host_converged=int(ref.converged.sum()),
                max_abs_theta_difference=float(np.abs(res.theta - ref.theta).max()))
    line["host_wall_over_fold_in_wall"] = line["host"]["wall"]["median_ms"] / \
        line["fold_in"]["wall"]["median_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=10_000)
    ap.add_argument("--rows-per-column", type=int, default=20)
    ap.add_argument("--row-nnz", type=int, default=30)
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name, lines=[])
    eng.close()
    rng = np.random.RandomState(0)
    d0, m = a.features, a.row_nnz - 1
    n = a.columns * a.rows_per_column
    # m distinct trained columns per row (a random start and a random odd stride), then the user
    start = rng.randint(0, d0, size=n)
    step = 1 + 2 * rng.randint(0, max(1, d0 // (2 * m)), size=n)
    other = np.sort((start[:, None] + step[:, None] * np.arange(m)[None, :]) % d0, axis=1)
    user = d0 + rng.permutation(np.repeat(np.arange(a.columns), a.rows_per_column))
    idx = np.concatenate([other, user[:, None]], axis=1)
    data = np.concatenate([rng.randn(n, m), np.ones((n, 1))], axis=1)
    X = sp.csr_matrix((data.ravel(), idx.ravel().astype(np.int32),
                       np.arange(0, n * (m + 1) + 1, m + 1, dtype=np.int64)),
                      shape=(n, d0 + a.columns))
    assert X.has_canonical_format
    cols = d0 + np.arange(a.columns)
    for degree, loss in ((2, "squared"), (3, "logistic")):
        line = _line(degree, loss, X, cols, a)
        res["lines"].append(line)
        print(json.dumps(line), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "foldin_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
