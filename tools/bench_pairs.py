"""Per-row pair attributions on the device against the per-entry attributions on the same rows.

Synthetic shape: 200 000 x 100 000, 50 entries per row (1 225 pairs per row), k = 30, f64 handle;
one line for degree 2 and one for degree 3 (fit_lower=None: one block each).  Per line, medians of
--repeats after --warmup calls:

  (a) pairs:         HipEngine.explain_pairs on the first --list-rows rows (a listing is capped at
                     1 GiB of values, so not all rows) -- the device time of its kernels
                     (spfm_explain_info: clearing the slab's values and the block kernel; not the
                     copies), also per million pairs, and the wall time of the whole call
  (b) pairs_topk:    HipEngine.explain_pairs_topk, K = 10, all rows -- device time (the block
                     kernel plus the per-row selection over the pair values) and wall time; only
                     n x K come back.  ``topk_select_ms`` is (b) minus (a) scaled to all rows.
  (c) explain:       HipEngine.explain (values + row sums) on all rows, device and wall: the
                     per-entry pass of the same run, the point of comparison

and the arithmetic the block kernel does per pair, k (2 + [M > 2] (2 + 3 (M - 2))) multiply-adds,
as a rate over the device time of (a).  Writes profiles/pairs_<build tag>.json unless --out is
given.  Nothing is asserted.

    python tools/bench_pairs.py [--rows 200000] [--features 100000] [--repeats 5] [--out FILE]
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
            dev.append(info()["device_ms"])
    return _median(dev), _median(wall)


def _line(degree, X, a):
    from sparsepoly_amd.engine import HipEngine

    rng = np.random.RandomState(degree)
    k, d, m = a.components, X.shape[1], a.row_nnz
    P = 0.1 * rng.randn(1, k, d)
    w = 0.1 * rng.randn(d)
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    blocks = [(0, degree)]
    coef = np.zeros((1, k, 7))
    coef[0, :, degree] = 1.0
    per_row = m * (m - 1) // 2
    Xl = X[:a.list_rows]
    line = dict(degree=degree, components=k, rows=X.shape[0], features=d, nnz=int(X.nnz), K=a.topk,
                n_pairs=X.shape[0] * per_row, list_rows=Xl.shape[0], list_pairs=Xl.shape[0] * per_row,
                fma_per_pair=k * (2 if degree == 2 else 4 + 3 * (degree - 2)))
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(P, w, lams)
        dev, wall = _timed(lambda: eng.explain_pairs(Xl, blocks, coef, True), eng.explain_info,
                           a.warmup, a.repeats)
        line["pairs"] = dict(device=dev, wall=wall, slabs=eng.explain_info()["slabs"],
                             device_ms_per_mpairs=dev["median_ms"] / (line["list_pairs"] / 1e6))
        dev_k, wall_k = _timed(lambda: eng.explain_pairs_topk(X, blocks, coef, True, a.topk),
                               eng.explain_info, a.warmup, a.repeats)
        line["pairs_topk"] = dict(device=dev_k, wall=wall_k, slabs=eng.explain_info()["slabs"])
        line["scratch_kib"] = eng.explain_info()["scratch_kib"]
        dev_e, wall_e = _timed(lambda: eng.explain(X, blocks, coef, True), eng.explain_info,
                               a.warmup, a.repeats)
        line["explain"] = dict(device=dev_e, wall=wall_e)
    finally:
        eng.close()
    block_all = dev["median_ms"] * line["n_pairs"] / line["list_pairs"]
    line["block_ms_all_rows"] = block_all
    line["topk_select_ms"] = dev_k["median_ms"] - block_all
    line["pairs_gfma_per_s"] = line["list_pairs"] * line["fma_per_pair"] / dev["median_ms"] / 1e6
    line["pairs_topk_device_over_explain_device"] = dev_k["median_ms"] / dev_e["median_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--row-nnz", type=int, default=50)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--list-rows", type=int, default=50_000)
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
    out = a.out or os.path.join(ROOT, "profiles", "pairs_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
