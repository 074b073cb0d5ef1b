#!/usr/bin/env python3
"""Write tests/golden/g12_interactions.npz: the reference fitted on the data of its
feature-interaction-selection example, and the selection metrics of the fitted blocks.

TEST INFRASTRUCTURE, like oracle/gen_golden.py: runs where the reference tree is on PYTHONPATH
behind ``oracle/numba_stub`` (identity ``@njit`` / ``@jitclass``: the reference's own source under
CPython, the same float64 operations in the same order):

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=oracle/numba_stub:<reference> \
        python3 tools/gen_golden_interactions.py [max_iter]

Data: RandomState(0), 200 samples of 100 features with a block covariance, a true pairwise
matrix ``W_true`` of eight 10 x 10 blocks of 0.5 without diagonal (its sum is 360.0), targets
``x^T W_true x`` plus noise.  Two fits with k = 30, ``mean=True``, ``fit_linear=False``:
squaredl12 / pcd (beta 0.2, gamma 0.1) and squaredl21 / pbcd (beta 0.2, gamma 1.0), ``max_iter``
iterations each (recorded).  Stored per fit: ``P_[0]``, ``lams_`` and the metrics of
``dense_metrics`` below -- a dense NumPy restatement in this project's words of what the example
measures (only inputs and outputs of the reference are stored, none of its text).
"""
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = (("sql12_pcd", "squaredl12", "pcd", 0.2, 0.1), ("sql21_pbcd", "squaredl21", "pbcd", 0.2, 1.0))
TOP = 50


def make_data():
    d, n = 100, 200
    rng = np.random.RandomState(0)
    W_true = np.zeros((d, d))
    cov = np.zeros((d, d))
    for lo in range(0, 80, 10):
        W_true[lo:lo + 10, lo:lo + 10] = 0.5
        cov[lo:lo + 10, lo:lo + 10] = 0.2
    np.fill_diagonal(W_true, 0.0)
    np.fill_diagonal(cov, 1.0)
    assert W_true.sum() == 360.0
    X = rng.multivariate_normal(np.zeros(d), cov, size=n)
    y = np.einsum("ij,jk,ik->i", X, W_true, X) + rng.normal(0, 0.1, n)
    return X, y, W_true


def dense_metrics(P, lams, W_true, top=TOP):
    """Pairs j < j' of W = P^T diag(lams) P (P is (k, d)) against W_true, W estimating 2 W_true:
    error (scaled), fscore, pssr, nnz, the non-zero pairs sorted by (row, col), and the `top`
    largest |W| by (|W| descending, row, column)."""
    W = P.T @ (lams[:, None] * P)
    iu = np.triu_indices(W.shape[0], k=1)
    we, wt = W[iu], W_true[iu]
    sel, true = we != 0, wt != 0
    tp, fp, fn = int((sel & true).sum()), int((sel & ~true).sum()), int((~sel & true).sum())
    precision = 0.0 if tp + fp == 0 else tp / (tp + fp)
    recall = 0.0 if tp + fn == 0 else tp / (tp + fn)
    fscore = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    error = np.sqrt(np.sum((2.0 * wt - we) ** 2)) / np.sqrt(np.sum((2.0 * wt) ** 2))
    rows, cols, vals = iu[0][sel], iu[1][sel], we[sel]
    order = np.lexsort((cols, rows, -np.abs(vals)))[:top]
    return dict(error=float(error), fscore=float(fscore), pssr=bool(fp + fn == 0),
                nnz=int(sel.sum()), tp=tp, fp=fp, fn=fn,
                rows=rows.astype(np.int32), cols=cols.astype(np.int32), vals=vals,
                top_rows=rows[order].astype(np.int32), top_cols=cols[order].astype(np.int32),
                top_vals=vals[order], sum_sq=float(np.sum(we ** 2)),
                sum_abs=float(np.sum(np.abs(we))), max_abs=float(np.abs(we).max(initial=0.0)))


def main():
    import sparsepoly  # the reference (via PYTHONPATH)
    from sparsepoly import SparseFactorizationMachineRegressor

    assert not os.path.abspath(sparsepoly.__file__).startswith(ROOT), sparsepoly.__file__
    max_iter = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    X, y, W_true = make_data()
    out = dict(X=X, y=y, W_true=W_true, max_iter=np.int64(max_iter))
    for name, reg, solver, beta, gamma in FITS:
        t0 = time.time()
        fm = SparseFactorizationMachineRegressor(
            n_components=30, fit_linear=False, beta=beta, gamma=gamma, regularizer=reg,
            solver=solver, mean=True, max_iter=max_iter, tol=1e-3, random_state=0, verbose=0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fm.fit(X, y)
        P, lams = np.ascontiguousarray(fm.P_[0]), np.asarray(fm.lams_, dtype=np.double)
        m = dense_metrics(P, lams, W_true)
        print("%s: %.0f s, error %.6f fscore %.6f pssr %d nnz %d" % (
            name, time.time() - t0, m["error"], m["fscore"], m["pssr"], m["nnz"]))
        out[name + "_P"] = P
        out[name + "_lams"] = lams
        for key, val in m.items():
            out[name + "_" + key] = np.asarray(val)
    path = os.path.join(ROOT, "tests", "golden", "g12_interactions.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
