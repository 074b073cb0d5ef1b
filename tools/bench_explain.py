"""Per-row attributions on the device against predict on the same rows.

Synthetic shape: 200 000 x 100 000, 50 entries per row, k = 30, f64 handle; one line for degree 2
and one for degree 3 (fit_lower=None: one block each).  Per line, medians of --repeats after
--warmup calls:

  (a) explain:       HipEngine.explain (values + row sums) -- the device time of its kernels
                     (spfm_explain_info: linear term, block kernel, row sums; not the copies) and
                     the wall time of the whole call, which copies nnz doubles back
  (b) explain_topk:  HipEngine.explain_topk, K = 10 -- device time (the same kernels plus the
                     per-row selection) and wall time; only n x K come back
  (c) predict:       the wall time of HipEngine.predict on the same rows, the point of comparison
                     (its kernel is the phase A of the block kernel without the table)

and the arithmetic the block kernel does, about 2 k M multiply-adds per entry over its two phases,
as a rate over the device time of (a).  Writes profiles/explain_<build tag>.json unless --out is
given.  Nothing is asserted.

    python tools/bench_explain.py [--rows 200000] [--features 100000] [--repeats 5] [--out FILE]
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


def _timed(call, info, warmup, repeats):
    dev, wall = [], []
    for rep in range(warmup + repeats):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if rep >= warmup:
            wall.append((t1 - t0) * 1e3)
            if info is not None:
                dev.append(info()["device_ms"])
    return (_median(dev) if dev else None), _median(wall)


def _line(degree, X, a):
    from sparsepoly_amd.engine import HipEngine

    rng = np.random.RandomState(degree)
    k, d = a.components, X.shape[1]
    P = 0.1 * rng.randn(1, k, d)
    w = 0.1 * rng.randn(d)
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    blocks = [(0, degree)]
    coef = np.zeros((1, k, 7))
    coef[0, :, degree] = 1.0
    line = dict(degree=degree, components=k, rows=X.shape[0], features=d, nnz=int(X.nnz), K=a.topk,
                fma_per_entry=2 * k * degree)
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(P, w, lams)
        dev, wall = _timed(lambda: eng.explain(X, blocks, coef, True), eng.explain_info, a.warmup,
                           a.repeats)
        line["explain"] = dict(device=dev, wall=wall, slabs=eng.explain_info()["slabs"])
        dev_k, wall_k = _timed(lambda: eng.explain_topk(X, blocks, coef, True, a.topk),
                               eng.explain_info, a.warmup, a.repeats)
        line["explain_topk"] = dict(device=dev_k, wall=wall_k)
        line["scratch_kib"] = eng.explain_info()["scratch_kib"]
        _, wall_p = _timed(lambda: eng.predict(X, degree, True, False), None, a.warmup, a.repeats)
        line["predict"] = dict(wall=wall_p)
    finally:
        eng.close()
    line["explain_gfma_per_s"] = line["nnz"] * line["fma_per_entry"] / dev["median_ms"] / 1e6
    line["explain_device_over_predict_wall"] = dev["median_ms"] / wall_p["median_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--row-nnz", type=int, default=50)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name, lines=[])
    eng.close()
    rng = np.random.RandomState(0)
    n, d, m = a.rows, a.features, a.row_nnz
    # m distinct columns per row: a random start and a random odd stride below d / m
    start = rng.randint(0, d, size=n)
    step = 1 + 2 * rng.randint(0, max(1, d // (2 * m)), size=n)
    cols = np.sort((start[:, None] + step[:, None] * np.arange(m)[None, :]) % d, axis=1)
    X = sp.csr_matrix((rng.randn(n * m), cols.ravel().astype(np.int32),
                       np.arange(0, n * m + 1, m, dtype=np.int64)), shape=(n, d))
    assert X.has_canonical_format
    for degree in (2, 3):
        line = _line(degree, X, a)
        res["lines"].append(line)
        print(json.dumps(line), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "explain_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
