"""A model bank against the same models' own decision_function calls.

Synthetic shape: F = 8 models with assigned parameters (degree 2, k = 30, linear term) over
d = 100 000 features, X of 1 000 000 rows x 50 entries, f64 handle.  Old and new alternate in one
process, warm, every call ending in a device synchronise; per side the median, minimum and maximum
wall time of --repeats rounds after --warmup:

  (old) solo:   est.decision_function(X) of the eight models one after the other -- _get_output:
                a handle, that model's parameters, X again, anova_predict_kernel, per model
  (new) bank:   ModelBank.decision_function / .argmax / .losses, the bank resident

Before any timing the (n, F) scores of the two sides are held equal within twice the bound of
tests/test_hip_bank.py at this size, (N + 2) 2^-53 S_hat with N = n_i + 2 M + 1 + k + 2 and S_hat
the bank of the models of magnitudes on |X| (computed on the device: its own error is of the order
of 1e-14 of it), and argmax / losses equal to what NumPy derives from the bank's own scores.

Bytes are counted from shapes, not measured: per stored entry 12 (column, value) + 8 S (the
stacked parameter row) + 8 F (the linear weights' row) and per row 8 (offset) + 8 F (scores) for
the bank, F x (2 x 12 + 8 k + 8) and F x 3 x 8 for the eight solo passes (their linear term is a
second sweep over the entries).  --profile-pass runs one round of each side and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_bank.py --profile-pass`; kernel times go
into the JSON by hand from that run's CSV (profiles/bank_<build tag>_kernel_stats.csv).

    python tools/bench_bank.py [--rows 1000000] [--repeats 5] [--out FILE]
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

U = 2.0 ** -53


def _stats(ts):
    ts = np.array(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                repeats=int(len(ts)))


def _models(F, k, d, degree):
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    ests = []
    for f in range(F):
        rng = np.random.RandomState(100 + f)
        est = SparseFactorizationMachineRegressor(degree=degree, n_components=k, fit_lower=None,
                                                  fit_linear=True, precision="f64", device=0)
        est.P_ = 0.1 * rng.randn(1, k, d)
        est.w_ = 0.1 * rng.randn(d)
        est.lams_ = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
        ests.append(est)
    return ests


def _matrix(n, d, m, seed=0):
    """m distinct columns per row: a random start and a random odd stride below d / m"""
    rng = np.random.RandomState(seed)
    start = rng.randint(0, d, size=n)
    step = 1 + 2 * rng.randint(0, max(1, d // (2 * m)), size=n)
    cols = np.sort((start[:, None] + step[:, None] * np.arange(m)[None, :]) % d, axis=1)
    X = sp.csr_matrix((rng.randn(n * m), cols.ravel().astype(np.int32),
                       np.arange(0, n * m + 1, m, dtype=np.int64)), shape=(n, d))
    assert X.has_canonical_format
    return X, np.where(rng.rand(n) < 0.5, -1.0, 1.0)


def _solo(ests, X):
    return np.stack([e.decision_function(X) if hasattr(e, "decision_function") else e.predict(X)
                     for e in ests], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--row-nnz", type=int, default=50)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import ModelBank, _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name)
    eng.close()
    F, k, d, m, n, M = a.models, a.components, a.features, a.row_nnz, a.rows, a.degree
    ests = _models(F, k, d, M)
    X, y = _matrix(n, d, m)
    S = F * k
    res.update(models=F, components=k, degree=M, rows=n, features=d, nnz=int(X.nnz),
               counted_bytes=dict(bank=int(X.nnz) * (12 + 8 * S + 8 * F) + n * (8 + 8 * F),
                                  solo=F * (int(X.nnz) * (2 * 12 + 8 * k + 8) + n * 3 * 8)))
    with ModelBank(ests) as bank:
        if a.profile_pass:
            _solo(ests, X)
            bank.decision_function(X)
            return
        # ---- agreement first
        import copy

        mags = []
        for e in ests:
            ab = copy.copy(e)
            ab.P_, ab.w_, ab.lams_ = np.abs(e.P_), np.abs(e.w_), np.ones_like(e.lams_)
            mags.append(ab)
        with ModelBank(mags) as ab_bank:
            S_hat = ab_bank.decision_function(abs(X)) * (1 + 1e-9)
        bound = (m + 2 * M + 1 + k + 2 + 2) * U * S_hat
        new, old = bank.decision_function(X), _solo(ests, X)
        worst = float((np.abs(new - old) / (2 * bound)).max())
        print("bank against solo: largest difference %.3g of twice the bound" % worst, flush=True)
        assert (np.abs(new - old) <= 2 * bound).all(), worst
        idx, best, runner = bank.argmax(X)
        assert (idx == new.argmax(axis=1)).all() and (best == new.max(axis=1)).all()
        assert (runner == np.sort(new, axis=1)[:, -2]).all()
        # loss sums from the same scores: 3 roundings of the loss and the device's sum
        # (20 + ceil(P / 256) additions over P blocks of 256 rows), + 2; the NumPy side adds in
        # longdouble (a float64 sum down the rows is n additions one after the other)
        ls = bank.losses(X, y, loss="squared")
        ref = (0.5 * (new - y[:, None]) ** 2).astype(np.longdouble).sum(axis=0)
        P = n // 256 + bank.info()["slabs"]
        worst_ls = float((np.abs(ls - ref) / ((3 + 20 + -(-P // 256) + 2) * U * ref)).max())
        print("loss sums: largest difference %.3g of the bound" % worst_ls, flush=True)
        assert worst_ls <= 1, (ls, ref)
        res.update(agreement_worst_fraction_of_twice_bound=worst, slabs=bank.info()["slabs"],
                   resident_bytes=bank.info()["resident_bytes"])
        # ---- old and new alternate
        calls = [("solo_8_decision_function", lambda: _solo(ests, X)),
                 ("bank_decision_function", lambda: bank.decision_function(X)),
                 ("bank_argmax", lambda: bank.argmax(X)),
                 ("bank_losses", lambda: bank.losses(X, y, loss="squared"))]
        times = {name: [] for name, _ in calls}
        for rep in range(a.warmup + a.repeats):
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if rep >= a.warmup:
                    times[name].append(t1 - t0)
        res["wall"] = {name: _stats(ts) for name, ts in times.items()}
    res["bank_over_solo_wall"] = (res["wall"]["bank_decision_function"]["median_ms"]
                                  / res["wall"]["solo_8_decision_function"]["median_ms"])
    out = a.out or os.path.join(ROOT, "profiles", "bank_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
