"""Average precision, best F1 and KS of a cross-validation grid: ModelBank.group_curve against
scores to the host and scikit-learn's curves.

The set-up of tools/bench_auc.py: 5 folds x 4 values of gamma = 20 members (degree 2, k = 30,
linear term) over d = 10 000 features, X of 100 000 rows x 50 entries, one row in ten positive,
f64 handle, one process.  Every member asks for two sets of rows: its held-out fold and the other
four.  The sides alternate, warm, every call ending in a device synchronise; per side the median,
minimum and maximum wall time of --repeats rounds after --warmup.

  (a) host:       bank.decision_function(X) -- the (n, F) scores come to the host -- then per
                  member and set scikit-learn's average_precision_score, the largest F1 of
                  precision_recall_curve and the largest |tpr - fpr| of roc_curve: what a user does
                  without ModelBank.group_curve
  (b) auc:        bank.group_auc(X, y, groups=fold, sets=[held, others]): its code is unchanged,
                  the yardstick inside the same run
  (c) curve:      bank.group_curve(...) with the same arguments
  (d) curve+auc:  bank.group_curve(..., auc=True): both tables from one pass and one sort per member
  (e) two calls:  bank.group_auc(...) followed by bank.group_curve(...)

(c) against (b) is what the second walk costs, (d) against (e) what sharing the pass and the sorts
saves.  Before any timing the unweighted integers and thresholds of (c) are held to
restate_group_curve on the bank's own scores (--check-members of them: its comparisons run in
Python integers), which must be equal, and the average precision to (4 n + 16) 2^-53 relative.

--profile-pass runs one group_auc, one group_curve and one group_curve(auc=True) pass and nothing
else, for `rocprofv3 --kernel-trace --stats -- python tools/bench_curve.py --profile-pass`.

    python tools/bench_curve.py [--rows 100000] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

U = 2.0 ** -53


def _host_side(scores, y, fold, held):
    """per member the held-out and the training (ap, best F1, ks), by scikit-learn on the host"""
    from sklearn.metrics import average_precision_score, precision_recall_curve, roc_curve

    pos = y > 0
    out = []
    for f in range(scores.shape[1]):
        s = scores[:, f] + 0.0
        own = fold == held[f]
        row = []
        for rows in (own, ~own):
            prec, rec, _ = precision_recall_curve(pos[rows], s[rows])
            with np.errstate(invalid="ignore", divide="ignore"):
                f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
            fpr, tpr, _ = roc_curve(pos[rows], s[rows], drop_intermediate=False)
            row.append((average_precision_score(pos[rows], s[rows]), f1.max(),
                        np.abs(tpr - fpr).max()))
        out.append(row)
    return np.array(out)


def main():
    from bench_bank import _matrix, _models, _stats

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=10_000)
    ap.add_argument("--row-nnz", type=int, default=50)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-members", type=int, default=2)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import ModelBank, _capi, fold_ids
    from sparsepoly_amd.bank import restate_group_curve
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name)
    eng.close()
    K, F, k, d, m, n, M = a.folds, a.folds * a.grid, a.components, a.features, a.row_nnz, a.rows, 2
    ests = _models(F, k, d, M)
    X, _ = _matrix(n, d, m)
    y = np.where(np.random.RandomState(2).rand(n) < 0.1, 1.0, -1.0)  # one row in ten is positive
    fold = fold_ids(n, K, random_state=0, stratify=y)
    held = np.tile(np.arange(K), a.grid)
    own = held[:, None] == np.arange(K)[None, :]
    sets = np.stack([own, ~own], axis=1)
    nb = -(-n // _capi.BANK_RANK_BLOCK)
    res.update(members=F, folds=K, grid=a.grid, components=k, degree=M, rows=n, features=d,
               nnz=int(X.nnz), precision="f64", sets_per_member=2,
               counted=dict(curve_walk_bytes=2 * 13 * n * F + 3 * 96 * nb * 2 * F,
                            curve_block_records_bytes=96 * nb * 2 * F,
                            resident_scratch_bytes=9 * n * F + 4 * n + 12 * n * F
                            + (40 + 96) * nb * 2 * F))
    kw = dict(groups=fold, n_groups=K, sets=sets)
    with ModelBank(ests, precision="f64") as bank:
        if a.profile_pass:
            bank.group_auc(X, y, **kw)
            bank.group_curve(X, y, **kw)
            bank.group_curve(X, y, auc=True, **kw)
            return
        # ---- agreement first
        scores = bank.decision_function(X)
        got = bank.group_curve(X, y, **kw)
        some = list(range(min(a.check_members, F)))
        want = restate_group_curve(scores[:, some], y, None, fold, K, sets[some])
        for name in ("counts", "f1_threshold", "ks_threshold", "best_f1", "ks"):
            assert np.array_equal(got[name][some], want[name], equal_nan=True), name
        ap_err = np.abs(got["average_precision"][some] - want["average_precision"])
        worst = float((ap_err / want["average_precision"]).max() / ((4 * n + 16) * U))
        assert worst <= 1, worst
        both = bank.group_curve(X, y, auc=True, **kw)
        auc = bank.group_auc(X, y, **kw)
        assert (both["pairs"] == auc["pairs"]).all() and (both["counts"] == got["counts"]).all()
        host = _host_side(scores[:, some], y, fold, held[some])
        dev = np.stack([got[name][some] for name in ("average_precision", "best_f1", "ks")], axis=2)
        host_diff = float(np.abs(dev - host).max())
        print("group_curve against the restatement: integers, thresholds, best_f1 and ks equal for "
              "%d members, average precision largest difference %.3g of the bound; against "
              "scikit-learn largest difference %.3g" % (len(some), worst, host_diff), flush=True)
        assert host_diff <= 1e-12, host_diff
        res.update(agreement_members_checked=len(some), agreement_integers_equal=True,
                   agreement_ap_worst_fraction_of_bound=worst,
                   agreement_sklearn_largest_difference=host_diff, slabs=bank.info()["slabs"],
                   mean_held_out_average_precision=float(got["average_precision"][:, 0].mean()))

        # ---- the five sides alternate
        def two_calls():
            bank.group_auc(X, y, **kw)
            bank.group_curve(X, y, **kw)

        calls = [("a_scores_to_host_then_sklearn",
                  lambda: _host_side(bank.decision_function(X), y, fold, held)),
                 ("b_bank_group_auc", lambda: bank.group_auc(X, y, **kw)),
                 ("c_bank_group_curve", lambda: bank.group_curve(X, y, **kw)),
                 ("d_bank_group_curve_with_auc", lambda: bank.group_curve(X, y, auc=True, **kw)),
                 ("e_group_auc_then_group_curve", two_calls)]
        times = {name: [] for name, _ in calls}
        for rep in range(a.warmup + a.repeats):
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if rep >= a.warmup:
                    times[name].append(t1 - t0)
        res["wall"] = {name: _stats(ts) for name, ts in times.items()}
    med = {name: v["median_ms"] for name, v in res["wall"].items()}
    res["c_over_a_median"] = med["c_bank_group_curve"] / med["a_scores_to_host_then_sklearn"]
    res["c_minus_b_median_ms"] = med["c_bank_group_curve"] - med["b_bank_group_auc"]
    res["d_minus_c_median_ms"] = med["d_bank_group_curve_with_auc"] - med["c_bank_group_curve"]
    res["d_over_e_median"] = (med["d_bank_group_curve_with_auc"]
                              / med["e_group_auc_then_group_curve"])

    out = a.out or os.path.join(ROOT, "profiles", "curve_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
