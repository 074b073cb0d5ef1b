"""ROC-AUC of a cross-validation grid: ModelBank.group_auc against scores to the host and argsort.

Synthetic shape, as tools/bench_cv.py: 5 folds x 4 values of gamma = 20 members (degree 2, k = 30,
linear term) over d = 10 000 features, X of 100 000 rows x 50 entries, f64 handle, one process.
Every member asks for two sets of rows: its held-out fold and the other four.  The sides alternate,
warm, every call ending in a device synchronise; per side the median, minimum and maximum wall time
of --repeats rounds after --warmup.

  (a) host:     bank.decision_function(X) -- the (n, F) scores come to the host -- then per member
                NumPy's stable argsort of the held-out rows and of the training rows and the
                tie-aware rank sum: the only route before ModelBank.group_auc
  (b) sums:     bank.group_sums(X, y, groups=fold, sample_weight=w) alone, for scale: the same
                scoring pass with a reduction that needs no sort
  (c) auc:      bank.group_auc(X, y, groups=fold, sets=[held, others]) -- unweighted, integers
  (d) auc_w:    the same with sample_weight=w -- doubles

Before any timing (c)'s pairs are held to (a)'s integers, which must be equal, and (d) to a
weighted host AUC within (4 n + 16) 2^-53 relative.

Counted from shapes, not measured, for (c) beyond the scoring pass: the key kernel reads 8 n F of
scores and writes 9 n F (keys, class and group bytes); one rocprim::radix_sort_pairs per member,
which up to 2^20 items (its merge_sort_limit) does not run radix passes but sorts blocks of 1024
pairs by radix and merges them: one block sort, ceil(log2(n / 1024)) merge passes and a copy back,
each reading and writing the 12 n bytes of the pairs -- 216 n bytes in 9 steps at n = 100 000 (the
kernel trace shows 1 + 7 + 2 launches per member).  Above 2^20 rows rocPRIM takes its radix passes
instead; not counted here.  The walk reads 12 n F + n F twice (two kernels) and gathers class
bytes (and weights).

--profile-pass runs one unweighted and one weighted group_auc pass and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_auc.py --profile-pass`.

    python tools/bench_auc.py [--rows 100000] [--repeats 5] [--out FILE]
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


def _host_auc(s, pos, w):
    """(U2 or 2 * numerator, W_pos, W_neg) of one score vector by a stable argsort: per tie run the
    positives times (negatives below + negatives through the run)"""
    order = np.argsort(s, kind="stable")
    s, pos = s[order], pos[order]
    wv = np.ones(len(s), dtype=np.int64) if w is None else w[order]
    tail = np.append(s[1:] != s[:-1], True)
    ninc = np.cumsum(np.where(pos, 0, wv))[tail]
    pinc = np.cumsum(np.where(pos, wv, 0))[tail]
    nst = np.concatenate([ninc[:1] * 0, ninc[:-1]])
    prun = np.diff(np.concatenate([pinc[:1] * 0, pinc]))
    return (prun * (nst + ninc)).sum(), pinc[-1], ninc[-1]


def _host_side(scores, y, fold, held, w):
    """per member the held-out and the training triple, from (n, F) scores on the host"""
    pos = y > 0
    out = []
    for f in range(scores.shape[1]):
        s = scores[:, f] + 0.0
        own = fold == held[f]
        out.append([_host_auc(s[rows], pos[rows], None if w is None else w[rows])
                    for rows in (own, ~own)])
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
    X, _ = _matrix(n, d, m)
    y = np.where(np.random.RandomState(2).rand(n) < 0.1, 1.0, -1.0)  # one row in ten is positive
    fold = fold_ids(n, K, random_state=0, stratify=y)
    w = np.random.RandomState(1).rand(n) + 0.5
    held = np.tile(np.arange(K), a.grid)
    own = held[:, None] == np.arange(K)[None, :]
    sets = np.stack([own, ~own], axis=1)
    nb = -(-n // _capi.BANK_RANK_BLOCK)
    merges = max(0, int(np.ceil(np.log2(n / 1024.0))))
    res.update(members=F, folds=K, grid=a.grid, components=k, degree=M, rows=n, features=d,
               nnz=int(X.nnz), precision="f64", sets_per_member=2,
               counted=dict(key_kernel_bytes=17 * n * F, sorts=F,
                            sort_path="block sort of 1024 pairs + merge passes + copy back "
                                      "(rocPRIM below its merge_sort_limit of 2^20 items)"
                            if n <= 1 << 20 else "radix passes: not counted",
                            sort_merge_passes_per_member=merges,
                            sort_bytes_per_member=24 * n * (2 + merges) if n <= 1 << 20 else None,
                            walk_bytes=2 * 13 * n * F + 2 * 40 * nb * 2 * F,
                            resident_scratch_bytes=9 * n * F + 4 * n + 12 * n * F
                            + 40 * nb * 2 * F))
    kw = dict(groups=fold, n_groups=K, sets=sets)
    with ModelBank(ests, precision="f64") as bank:
        if a.profile_pass:
            bank.group_auc(X, y, **kw)
            bank.group_auc(X, y, sample_weight=w, **kw)
            return
        # ---- agreement first
        scores = bank.decision_function(X)
        want = _host_side(scores, y, fold, held, None)
        got = bank.group_auc(X, y, **kw)
        assert (got["pairs"] == want.astype(np.int64)).all()
        want_w = _host_side(scores, y, fold, held, w.astype(np.longdouble))
        got_w = bank.group_auc(X, y, sample_weight=w, **kw)
        auc_w = (want_w[:, :, 0] / 2 / (want_w[:, :, 1] * want_w[:, :, 2])).astype(np.double)
        worst = float((np.abs(got_w["auc"] - auc_w) / auc_w).max() / ((4 * n + 16) * U))
        print("group_auc against the host route: integers equal, weighted largest difference "
              "%.3g of the bound" % worst, flush=True)
        assert worst <= 1, worst
        res.update(agreement_pairs_equal=True, agreement_weighted_worst_fraction_of_bound=worst,
                   slabs=bank.info()["slabs"],
                   mean_held_out_auc=float(got["auc"][:, 0].mean()))

        # ---- the four sides alternate
        calls = [("a_scores_to_host_then_argsort",
                  lambda: _host_side(bank.decision_function(X), y, fold, held, None)),
                 ("b_bank_group_sums", lambda: bank.group_sums(
                     X, y, groups=fold, n_groups=K, sample_weight=w, metrics=("logistic",))),
                 ("c_bank_group_auc", lambda: bank.group_auc(X, y, **kw)),
                 ("d_bank_group_auc_weighted", lambda: bank.group_auc(X, y, sample_weight=w, **kw))]
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
    res["c_over_a_median"] = med["c_bank_group_auc"] / med["a_scores_to_host_then_argsort"]
    res["d_over_a_median"] = med["d_bank_group_auc_weighted"] / med["a_scores_to_host_then_argsort"]
    res["c_minus_b_median_ms"] = med["c_bank_group_auc"] - med["b_bank_group_sums"]

    out = a.out or os.path.join(ROOT, "profiles", "auc_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
