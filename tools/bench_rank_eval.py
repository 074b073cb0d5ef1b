"""Full-catalogue evaluation on the device (Ranker.evaluate) against the dense-scores route.

Shape of tools/bench_rank.py: k = 30, C = 100 000 one-feature candidates, B = 8192 contexts of 30
non-zeros, f64 handle; one line for degree 2 and one for degree 3 with fit_lower='explicit'
(R = 90).  Per context row 5 targets and 50 excluded candidates, drawn without replacement.  Per
line:

  (a) kernels:  device time (spfm_rank_info) of the kernels of `evaluate` -- context towers, target
                scores, count pass -- next to that of top_k(K = 100), with and without the same
                exclusion lists, at the same shape in the same process; medians of --repeats after
                --warmup calls, every call ending in a synchronise (the calls return host arrays)
  (b) wall:     Ranker.evaluate against the only route without it: ranker.scores in row chunks
                under the 1 GiB cap, then NumPy ranks by the definition (excluded columns set to
                -inf, per target one `>` count and one `==` count over the lower indices), once
  (c) equal:    the number of rows on which the two routes give the same ranks, and the total

Writes profiles/rank_eval_<build tag>.json unless --out is given.  Nothing is asserted.

    python tools/bench_rank_eval.py [--contexts 8192] [--candidates 100000] [--repeats 5]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_rank import _median, _problem  # noqa: E402


def _lists(B, C, n_targets, n_excluded, seed):
    """(B, C) CSR patterns of targets and excluded candidates, disjoint per row"""
    rng = np.random.RandomState(seed)
    n = n_targets + n_excluded
    pick = np.empty((B, n), dtype=np.int64)
    draw = rng.randint(C, size=(B, 2 * n)) if C >= 64 * n else None
    for b in range(B):
        if draw is None:
            pick[b] = rng.choice(C, size=n, replace=False)
            continue
        _, first = np.unique(draw[b], return_index=True)  # the first n distinct draws
        pick[b] = draw[b][np.sort(first)[:n]]
    rows = np.arange(B)

    def mat(cols):
        m = sp.csr_matrix((np.ones(cols.size), (np.repeat(rows, cols.shape[1]), cols.ravel())),
                          shape=(B, C))
        m.sort_indices()
        return m

    return mat(pick[:, :n_targets]), mat(pick[:, n_targets:])


def _dense_route(ranker, X, T, E, budget):
    """ranks by the definition from dense score chunks; -> (ranks aligned with T, seconds of
    the device calls, seconds of NumPy)"""
    B, C = T.shape
    chunk = max(1, int(budget // (8 * C)))
    ranks = np.empty(T.nnz, dtype=np.int32)
    t_scores = t_numpy = 0.0
    for r0 in range(0, B, chunk):
        t0 = time.perf_counter()
        S = ranker.scores(X[r0:r0 + chunk])
        t1 = time.perf_counter()
        for i in range(S.shape[0]):
            b = r0 + i
            row = S[i]
            tt = T.indices[T.indptr[b]:T.indptr[b + 1]]
            s = row[tt].copy()
            row[E.indices[E.indptr[b]:E.indptr[b + 1]]] = -np.inf
            row[~np.isfinite(row)] = -np.inf
            for j, (t, v) in enumerate(zip(tt, s)):
                ranks[T.indptr[b] + j] = ((row > v).sum() + (row[:t] == v).sum()
                                          if np.isfinite(v) else -1)
        t2 = time.perf_counter()
        t_scores += t1 - t0
        t_numpy += t2 - t1
    return ranks, t_scores, t_numpy


def _line(degree, a):
    from sparsepoly_amd import _capi

    k, B, C, K = a.components, a.contexts, a.candidates, a.topk
    est, X, Z = _problem(degree, k, B, C, a.context_features, a.context_nnz, seed=degree)
    T, E = _lists(B, C, a.targets, a.excluded, seed=100 + degree)
    R = k * (degree - 1) + (k if degree == 3 else 0)
    line = dict(degree=degree, components=k, contexts=B, candidates=C, K=K, tower_columns=R,
                context_nnz=a.context_nnz, targets_per_row=a.targets, excluded_per_row=a.excluded)
    ranker = est.ranker(Z)
    eng = ranker._engine
    calls = dict(evaluate=lambda: ranker.evaluate(X, T, E, ks=(10,)),
                 evaluate_no_exclusions=lambda: ranker.evaluate(X, T, None, ks=(10,)),
                 top_k=lambda: ranker.top_k(X, K),
                 top_k_excluding=lambda: ranker.top_k(X, K, exclude=E))
    for name, call in calls.items():
        dev, wall = [], []
        for rep in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            out = call()
            t1 = time.perf_counter()
            if rep >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                dev.append(eng.rank_info()["device_ms"])
        line[name] = dict(kernels=_median(dev), wall=_median(wall))
        if name == "evaluate":
            line["metrics"] = {m: v for m, v in out.items() if m != "per_row"}
    line["kernels_evaluate_over_top_k"] = (line["evaluate"]["kernels"]["median_ms"]
                                           / line["top_k"]["kernels"]["median_ms"])
    line["scratch_kib"] = eng.rank_info()["scratch_kib"]
    ranks, _ = ranker.ranks(X, T, E)

    t0 = time.perf_counter()
    want, t_scores, t_numpy = _dense_route(ranker, X, T, E, _capi.RANK_SCORES_MAX_BYTES)
    total = (time.perf_counter() - t0) * 1e3
    ranker.close()
    same = np.add.reduceat((ranks == want).astype(np.int64), T.indptr[:-1]) == np.diff(T.indptr)
    line["dense_route"] = dict(wall_ms=total, scores_calls_ms=t_scores * 1e3,
                               numpy_ranks_ms=t_numpy * 1e3, repeats=1,
                               chunks=int(-(-B // max(1, _capi.RANK_SCORES_MAX_BYTES // (8 * C)))))
    line["ratio_dense_route_to_evaluate_wall"] = total / line["evaluate"]["wall"]["median_ms"]
    line["rows_with_equal_ranks"] = int(same.sum())
    line["rows"] = B
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=8192)
    ap.add_argument("--candidates", type=int, default=100_000)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--targets", type=int, default=5)
    ap.add_argument("--excluded", type=int, default=50)
    ap.add_argument("--context-features", type=int, default=2000)
    ap.add_argument("--context-nnz", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name, lines=[])
    eng.close()
    for degree in (2, 3):
        line = _line(degree, a)
        res["lines"].append(line)
        print(json.dumps(line), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "rank_eval_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
