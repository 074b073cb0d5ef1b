"""Candidate ranking on the device against a host recipe and against predict on stacked rows.

Flagship shape: degree 2, k = 30, C = 100 000 one-feature candidates, B = 8192 contexts of 30
non-zeros, K = 100; plus one degree-3 line with fit_lower='explicit' (R = 90).  Per line:

  (a) device:  Ranker.top_k -- the device time of its kernels (spfm_rank_info: towers of the
               contexts, score tiles with the per-row selection, merge) and the wall time of the
               whole call; medians of --repeats; the fraction of the arithmetic bound 2 B C R flops
               at 78.6 TFLOP/s (f64 matrix rate) that the device time is
  (b) host:    NumPy on the same towers (less the columns that are identically zero for
               one-feature candidates), U @ V.T + argpartition + sort of the K, in row blocks, on
               16 threads, once; its indices are compared with the device's (reported, not asserted)
  (c) parent:  the only route without this feature, est.predict on the stacked rows x_b + z_c,
               timed on a slice of at most --pairs (context, candidate) pairs and scaled by the
               pair count: marked "scaled"

Writes profiles/rank_<build tag>.json unless --out is given.  Nothing is asserted.

    python tools/bench_rank.py [--contexts 8192] [--candidates 100000] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_FLOPS = 78.6e12


def _median(ts):
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                repeats=int(len(ts)))


def _problem(degree, k, B, C, dc, nnz, seed):
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    rng = np.random.RandomState(seed)
    d = dc + C
    est = SparseFactorizationMachineRegressor(degree=degree, n_components=k, fit_lower="explicit",
                                              fit_linear=True, precision="f64")
    est.P_ = 0.1 * rng.randn(degree - 1, k, d)
    est.w_ = 0.1 * rng.randn(d)
    est.lams_ = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    cols = np.argsort(rng.rand(B, dc), axis=1)[:, :nnz].ravel()
    X = sp.csr_matrix((rng.randn(B * nnz), (np.repeat(np.arange(B), nnz), cols)), shape=(B, d))
    Z = sp.csr_matrix((0.5 + rng.rand(C), (np.arange(C), dc + np.arange(C))), shape=(C, d))
    return est, X, Z


def _host_towers(est, X, Z, dc):
    """rowconst, colconst, U, V for one-feature candidates (a^t(z) = 0 for t >= 2)"""
    degree, lams, w = est.degree, est.lams_, est.w_
    zval = Z.data
    Xc = X[:, :dc]

    def ctx_kernels(P, m):  # a^1..a^m of the contexts by Newton's identities, (B, k) each
        pw = [None] + [np.asarray((Xc.power(t) if t > 1 else Xc) @ (P[:, :dc] ** t).T)
                       for t in range(1, m + 1)]
        a = [np.ones_like(pw[1])]
        for t in range(1, m + 1):
            a.append(sum((-1) ** (i - 1) * a[t - i] * pw[i] for i in range(1, t + 1)) / t)
        return a

    a = ctx_kernels(est.P_[0], degree)
    rowc = np.asarray(Xc @ w[:dc]).ravel() + (a[degree] * lams).sum(axis=1)
    colc = w[dc:] * zval
    # cross terms: only a^1(z) = p z is non-zero, so t = degree - 1 survives in the top block
    U = [a[degree - 1] * lams]
    V = [(est.P_[0][:, dc:] * zval).T]
    if degree == 3:  # the order-2 term on P_[1]
        a_low = ctx_kernels(est.P_[1], 2)
        rowc = rowc + (a_low[2] * lams).sum(axis=1)
        U.append(a_low[1] * lams)
        V.append((est.P_[1][:, dc:] * zval).T)
    return rowc, colc, np.hstack(U), np.ascontiguousarray(np.hstack(V))


def _host_topk(rowc, colc, U, V, K, block=256):
    B = U.shape[0]
    idx = np.empty((B, K), dtype=np.int32)
    for r0 in range(0, B, block):
        S = U[r0:r0 + block] @ V.T
        S += rowc[r0:r0 + block, None]
        S += colc[None, :]
        part = np.argpartition(-S, K - 1, axis=1)[:, :K]
        vals = np.take_along_axis(S, part, axis=1)
        order = np.lexsort((part, -vals), axis=1)
        idx[r0:r0 + block] = np.take_along_axis(part, order, axis=1)
    return idx


def _line(degree, a):
    from sparsepoly_amd import _capi  # noqa: F401

    k, B, C, K = a.components, a.contexts, a.candidates, a.topk
    est, X, Z = _problem(degree, k, B, C, a.context_features, a.context_nnz, seed=degree)
    R = k * (degree - 1) + (k if degree == 3 else 0)  # degree 3: + the order-2 block
    bound_ms = 2.0 * B * C * R / F64_MATRIX_FLOPS * 1e3
    line = dict(degree=degree, components=k, contexts=B, candidates=C, K=K, tower_columns=R,
                context_nnz=a.context_nnz, bound_ms=bound_ms)
    t0 = time.perf_counter()
    ranker = est.ranker(Z)
    line["set_candidates_ms"] = (time.perf_counter() - t0) * 1e3
    eng = ranker._engine
    Xa = sp.csr_matrix(X)
    dev, wall, call = [], [], []
    idx = None
    for rep in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        idx, val = ranker.top_k(X, K)
        t1 = time.perf_counter()
        eng.rank_topk(Xa, K)  # the engine call alone: no input checks of the Python layer
        t2 = time.perf_counter()
        if rep >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            call.append((t2 - t1) * 1e3)
            dev.append(eng.rank_info()["device_ms"])
    line["device"] = _median(dev)
    line["engine_call"] = _median(call)
    line["ranker_top_k"] = _median(wall)
    line["fraction_of_bound"] = bound_ms / line["device"]["median_ms"]
    line["scratch_kib"] = eng.rank_info()["scratch_kib"]
    ranker.close()

    t0 = time.perf_counter()
    rowc, colc, U, V = _host_towers(est, X, Z, a.context_features)
    t1 = time.perf_counter()
    hidx = _host_topk(rowc, colc, U, V, K)
    t2 = time.perf_counter()
    line["host"] = dict(towers_ms=(t1 - t0) * 1e3, product_topk_ms=(t2 - t1) * 1e3, repeats=1,
                        threads=int(os.environ["OMP_NUM_THREADS"]),
                        rows_equal_to_device=int((hidx == idx).all(axis=1).sum()))

    nb = max(1, min(B, int(a.pairs // C)))
    Xs = X[np.repeat(np.arange(nb), C)] + sp.vstack([Z] * nb).tocsr()
    ts = []
    for rep in range(1 + min(a.repeats, 3)):
        t0 = time.perf_counter()
        est.predict(Xs)
        if rep:
            ts.append((time.perf_counter() - t0) * 1e3)
    par = _median(ts)
    par.update(pairs_timed=nb * C, scaled=True,
               scaled_to_all_pairs_ms=par["median_ms"] * (B * C) / float(nb * C))
    line["parent_predict_stacked"] = par
    line["ratio_parent_scaled_to_ranker_top_k"] = (par["scaled_to_all_pairs_ms"]
                                                   / line["ranker_top_k"]["median_ms"])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=8192)
    ap.add_argument("--candidates", type=int, default=100_000)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--context-features", type=int, default=2000)
    ap.add_argument("--context-nnz", type=int, default=30)
    ap.add_argument("--pairs", type=float, default=4e5,
                    help="(context, candidate) pairs of the stacked-predict slice, at most 2e6")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.pairs = min(a.pairs, 2e6)

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name,
               f64_matrix_flops=F64_MATRIX_FLOPS, lines=[])
    eng.close()
    for degree in (2, 3):
        line = _line(degree, a)
        res["lines"].append(line)
        print(json.dumps(line), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "rank_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
