"""Scoring a cross-validation grid: one grouped pass of a model bank against the per-member route.

Synthetic shape: 5 folds x 4 values of gamma = 20 members (degree 2, k = 30, linear term) over
d = 10 000 features, X of 100 000 rows x 50 entries, f64 handle, one process.  The sides alternate,
warm, every call ending in a device synchronise; per side the median, minimum and maximum wall time
of --repeats rounds after --warmup.

Scoring (members with assigned parameters: the passes do not care where they came from):
  (a) solo:    per member est.predict(X), then the masked NumPy loss per fold -- the only way
               before ModelBank.group_sums
  (b) losses:  bank.losses(X, y) of the same bank: ungrouped, unweighted, its own two kernels
  (c) groups:  one bank.group_sums(X, y, groups=fold, sample_weight=w) pass

Before any timing (c)'s table is held to (a)'s values within the bound of
tests/test_hip_bank_groups.py at this size: both sides' scores are within b = (N + 2) 2^-53 S_hat
of the exact ones (N = n_i + 2 M + 1 + k + 2, S_hat from the bank of magnitudes on |X|, computed on
the device), so the cells differ by at most 2 sum w_i terms_i + (N_sum + 3 + 3) 2^-53 sum w_i
loss_i, N_sum = 64 + 4 + P, P the call's blocks of 256 rows (3: the roundings of NumPy's own loss;
its sums are taken in longdouble).

Bytes are counted from shapes, not measured: the scoring pass reads per stored entry 12 + 8 S + 8 F
and per row 8 + 8 F (bank_predict_kernel, unchanged), the reduction behind it n F 8 of scores and
8 n of targets; the grouped one reads 12 n more (ids and weights).  Expectation: (c) within (b)
plus the larger of (b)'s own min-max spread and the share of those 12 n bytes.

End to end (--end-to-end): cross_validate_path against fit_concurrently with masks followed by
side (a), --fit-epochs epochs of pcd per clone, f32 storage for the fits as the estimators default.

--profile-pass runs one group_sums pass and one losses pass and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_cv.py --profile-pass`.

    python tools/bench_cv.py [--rows 100000] [--repeats 5] [--end-to-end] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

U = 2.0 ** -53


def _masked_losses(scores, y, w, fold, K):
    """(F, K) weighted squared-loss sums of (n, F) scores per fold, summed in longdouble"""
    vals = (w[:, None] * (0.5 * (scores - y[:, None]) ** 2)).astype(np.longdouble)
    return np.stack([vals[fold == g].sum(axis=0) for g in range(K)], axis=1)


def main():
    from bench_bank import _matrix, _models, _solo, _stats

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=10_000)
    ap.add_argument("--row-nnz", type=int, default=50)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--fit-epochs", type=int, default=2)
    ap.add_argument("--e2e-repeats", type=int, default=2)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import ModelBank, _capi, fold_ids
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name)
    eng.close()
    K, F, k, d, m, n, M = a.folds, a.folds * a.grid, a.components, a.features, a.row_nnz, a.rows, 2
    ests = _models(F, k, d, M)
    X, y = _matrix(n, d, m)
    fold = fold_ids(n, K, random_state=0)
    w = np.random.RandomState(1).rand(n) + 0.5
    S = F * k
    predict_bytes = int(X.nnz) * (12 + 8 * S + 8 * F) + n * (8 + 8 * F)
    reduce_bytes = n * F * 8 + n * 8
    res.update(members=F, folds=K, grid=a.grid, components=k, degree=M, rows=n, features=d,
               nnz=int(X.nnz), precision="f64",
               counted_bytes=dict(predict=predict_bytes, losses_reduction=reduce_bytes,
                                  groups_reduction=reduce_bytes + 12 * n))
    with ModelBank(ests, precision="f64") as bank:
        if a.profile_pass:
            bank.group_sums(X, y, groups=fold, n_groups=K, sample_weight=w, metrics=("squared",))
            bank.losses(X, y, loss="squared")
            return
        # ---- agreement first
        import copy

        mags = []
        for e in ests:
            ab = copy.copy(e)
            ab.P_, ab.w_, ab.lams_ = np.abs(e.P_), np.abs(e.w_), np.ones_like(e.lams_)
            mags.append(ab)
        with ModelBank(mags, precision="f64") as ab_bank:
            S_hat = ab_bank.decision_function(abs(X)) * (1 + 1e-9)
        b = ((m + 2 * M + 1 + k + 2 + 2) * U * S_hat).astype(np.longdouble)
        old = _solo(ests, X)
        tab_a = _masked_losses(old, y, w, fold, K)
        got = bank.group_sums(X, y, groups=fold, n_groups=K, sample_weight=w,
                              metrics=("squared",))
        slabs = bank.info()["slabs"]
        P = -(-n // 256) + slabs
        r = (np.abs(old) + np.abs(y)[:, None]).astype(np.longdouble)
        terms = b * (r + b / 2) + 3 * U * 0.5 * (r + b) ** 2  # _loss_terms('squared', ...)
        wl = w.astype(np.longdouble)[:, None]
        tol = np.stack([(2 * wl * terms)[fold == g].sum(axis=0) for g in range(K)], axis=1) \
            + (64 + 4 + P + 3 + 3) * U * tab_a
        worst = float((np.abs(got["squared"] - tab_a) / tol).max())
        print("group_sums against the solo route: largest difference %.3g of the bound" % worst,
              flush=True)
        assert worst <= 1, worst
        res.update(agreement_worst_fraction_of_bound=worst, slabs=slabs)

        # ---- the three sides alternate
        def side_a():
            return _masked_losses(_solo(ests, X), y, w, fold, K)

        calls = [("a_solo_predict_then_numpy", side_a),
                 ("b_bank_losses", lambda: bank.losses(X, y, loss="squared")),
                 ("c_bank_group_sums", lambda: bank.group_sums(
                     X, y, groups=fold, n_groups=K, sample_weight=w, metrics=("squared",)))]
        times = {name: [] for name, _ in calls}
        for rep in range(a.warmup + a.repeats):
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if rep >= a.warmup:
                    times[name].append(t1 - t0)
        res["wall"] = {name: _stats(ts) for name, ts in times.items()}
    wb, wc = res["wall"]["b_bank_losses"], res["wall"]["c_bank_group_sums"]
    spread = (wb["max_ms"] - wb["min_ms"]) / wb["median_ms"]
    share = 12.0 * n / (predict_bytes + reduce_bytes + 12 * n)
    res["expectation"] = dict(
        b_spread=spread, extra_bytes_share=share,
        c_over_b_median=wc["median_ms"] / wb["median_ms"],
        c_within_b_plus_margin=bool(wc["median_ms"] <= wb["median_ms"] * (1 + max(spread, share))))
    res["c_over_a_median"] = wc["median_ms"] / res["wall"]["a_solo_predict_then_numpy"]["median_ms"]

    if a.end_to_end:
        from sklearn.base import clone

        from sparsepoly_amd import SparseFactorizationMachineRegressor, cross_validate_path
        from sparsepoly_amd.concurrent import fit_concurrently

        base = SparseFactorizationMachineRegressor(
            degree=2, n_components=k, solver="pcd", schedule="colored", max_iter=a.fit_epochs,
            tol=0, random_state=0, alpha=1e-3, beta=1e-3, gamma=1e-3, device=0)
        gammas = [10.0 ** -(i + 1) for i in range(a.grid)]

        def parent_recipe():
            clones = [clone(base).set_params(gamma=g) for g in gammas for _ in range(K)]
            masks = [(fold != f) * w for _ in gammas for f in range(K)]
            fit_concurrently(clones, X, y, sample_weights=masks)
            return _masked_losses(_solo(clones, X), y, w, fold, K)

        def new_call():
            return cross_validate_path(base, X, y, cv=fold, sample_weight=w, gamma=gammas)

        e2e = {"parent_fit_concurrently_then_solo": [], "cross_validate_path": []}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for rep in range(1 + a.e2e_repeats):
                for name, call in (("parent_fit_concurrently_then_solo", parent_recipe),
                                   ("cross_validate_path", new_call)):
                    t0 = time.perf_counter()
                    call()
                    t1 = time.perf_counter()
                    if rep >= 1:
                        e2e[name].append(t1 - t0)
        res["end_to_end"] = dict(fit_epochs=a.fit_epochs, fit_precision="f32",
                                 wall={name: _stats(ts) for name, ts in e2e.items()})

    out = a.out or os.path.join(ROOT, "profiles", "cv_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
