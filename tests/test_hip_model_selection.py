"""``cross_validate_path`` on the device.  Needs a real MI355X: ``pytest -m gpu``.

Small fits, as ``test_folds_on_one_image``: 400 x 60 at 5 entries per row, ``k = 4``, 4 epochs,
f32 storage (``X`` is rounded to float32 first, so the fits, the bank and NumPy see the same
inputs).  The fitted clones are held to their solo fits bit for bit; the scores are compared with
the NumPy metric of each clone's restated scores.  The bound of a table cell is the one of
``tests/test_hip_bank_groups.py`` (400 rows: P = 2 blocks, ``N_sum = 64 + 4 + 2``).  A held-out
score is one cell divided by the fold's weight (the test divides by the same double): one more
rounding.  A training score adds K - 1 cells in ascending fold order (at most K - 2 further
additions on a cell) and divides: ``(sum of the cells' bounds + (K + 1) 2^-53 sum of the cells) /
weight``.
"""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from test_hip_bank import CLEAR, U, _loss_terms, _reference

pytestmark = pytest.mark.gpu

N, D = 400, 60
N_SUM = 64 + 4 + 2


def _problem(seed=11):
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(N, D, 5, seed=seed)
    X = sp.csr_matrix(X)
    X.data = X.data.astype(np.float32).astype(np.float64)
    return X, np.asarray(y, dtype=np.float64)


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def _same_bits(a, b):
    np.testing.assert_array_equal(a.P_, b.P_)
    np.testing.assert_array_equal(a.lams_, b.lams_)
    if hasattr(a, "w_"):
        np.testing.assert_array_equal(a.w_, b.w_)


def _cells(est, X, y, w, fold, K, loss):
    """per fold the exact weighted loss sum of one clone's restated scores and its bound, the
    restated scores and their bound"""
    from sparsepoly_amd.bank import _metric

    want, bound, _ = _reference([est], X)
    vals = _metric(loss, want[:, 0], y, np.longdouble)
    terms = _loss_terms(loss, want[:, 0], y, bound[:, 0])
    wl = w.astype(np.longdouble)
    exact = np.array([(wl * vals)[fold == g].sum() for g in range(K)], dtype=np.longdouble)
    tol = np.array([(wl * terms)[fold == g].sum() for g in range(K)], dtype=np.longdouble)
    return exact, tol + (N_SUM + 3) * U * exact, want[:, 0], bound[:, 0]


def _check_scores(res, X, y, w, loss, what):
    """test_['loss'] and train_['loss'] of every clone against its restated scores; returns the
    restated (mean test loss, its bound) per grid point"""
    K = res.n_folds_
    weight = np.bincount(res.fold_, weights=w, minlength=K)
    worst = 0.0
    means = []
    for p in range(len(res.params)):
        mean, mean_tol = np.longdouble(0), np.longdouble(0)
        for f in range(K):
            exact, tol, _, _ = _cells(res.estimators_[p][f], X, y, w, res.fold_, K, loss)
            want = exact[f] / weight[f]
            lim = tol[f] / weight[f] + U * want
            err = abs(res.test_["loss"][p, f] - want)
            worst = max(worst, float(err / lim))
            assert err <= lim, (what, "test", p, f, float(err / lim))
            mean, mean_tol = mean + want / K, mean_tol + lim / K
            den = 0.0
            for g in range(K):  # the same doubles in the same order as the result's own
                if g != f:
                    den += weight[g]
            others = [g for g in range(K) if g != f]
            want = exact[others].sum() / den
            lim = (tol[others].sum() + (K + 1) * U * exact[others].sum()) / den
            err = abs(res.train_["loss"][p, f] - want)
            worst = max(worst, float(err / lim))
            assert err <= lim, (what, "train", p, f, float(err / lim))
        means.append((mean, mean_tol + (K + 1) * U * mean))
    print("%s: largest error %.3g of its bound" % (what, worst))
    return means


@pytest.fixture(scope="module")
def regression():
    """pcd, K = 4, two values of gamma, refit: run once"""
    from sparsepoly_amd import SparseFactorizationMachineRegressor, cross_validate_path

    X, y = _problem()
    base = SparseFactorizationMachineRegressor(solver="pcd", schedule="colored", max_iter=4, tol=0,
                                               random_state=0, gamma=1e-3, beta=1e-3, alpha=1e-3,
                                               n_components=4, precision="f32")
    fold = (np.arange(N) % 4).astype(np.int32)
    res = _quiet(cross_validate_path, base, X, y, cv=fold, refit=True, gamma=[1e-3, 30.0])
    return base, X, y, fold, res


def test_regressor_clones_equal_their_solo_fits(regression):
    from sklearn.base import clone

    base, X, y, fold, res = regression
    assert res.params == [{"gamma": 1e-3}, {"gamma": 30.0}] and (res.fold_ == fold).all()
    assert res.info_ == dict(banks=1, passes=1, members=[8])
    for p, params in enumerate(res.params):
        for f in range(4):
            solo = _quiet(clone(base).set_params(**params).fit, X, y,
                          sample_weight=(fold != f).astype(np.float64))
            _same_bits(res.estimators_[p][f], solo)
    assert not np.array_equal(res.estimators_[0][0].P_, res.estimators_[0][1].P_)


def test_regressor_scores_and_the_best_index(regression):
    from sklearn.base import clone

    base, X, y, fold, res = regression
    assert set(res.test_) == {"loss"} and res.test_["loss"].shape == (2, 4)
    means = _check_scores(res, X, y, np.ones(N), "squared", "regressor, pcd")
    np.testing.assert_array_equal(res.mean_test_["loss"], res.test_["loss"].mean(axis=1))
    np.testing.assert_array_equal(res.std_test_["loss"], res.test_["loss"].std(axis=1))
    # the restated side first: the two mean test losses are further apart than their bounds
    (m0, t0), (m1, t1) = means
    assert abs(m0 - m1) > t0 + t1
    best = 0 if m0 < m1 else 1
    assert res.best_index_ == best and res.best_params_ == res.params[best]
    solo = _quiet(clone(base).set_params(**res.params[best]).fit, X, y)
    _same_bits(res.best_estimator_, solo)


def test_classifier_pbcd_logistic_stratified_with_weights():
    from sparsepoly_amd import (SparseFactorizationMachineClassifier, cross_validate_path,
                                fold_ids)
    from sparsepoly_amd.bank import restate_group_sums

    X, y = _problem(seed=12)
    labels = np.where(y > np.median(y), "pos", "neg")
    pm = np.where(labels == "pos", 1.0, -1.0)
    rng = np.random.RandomState(3)
    w = rng.randint(0, 3, size=N).astype(np.float64)  # integer weights, zeros among them
    assert (w == 0).any()
    base = SparseFactorizationMachineClassifier(
        solver="pbcd", loss="logistic", regularizer="omegacs", schedule="colored", max_iter=4,
        tol=0, random_state=5, beta=1e-3, gamma=1e-3, alpha=1e-3, n_components=4, precision="f32")
    res = _quiet(cross_validate_path, base, X, labels, cv=3, sample_weight=w,
                 beta=[1e-3, 1e-1], keep_estimators=True)
    assert (res.fold_ == fold_ids(N, 3, random_state=5, stratify=labels)).all()
    assert set(res.test_) == {"loss", "sign_error"} and res.info_["passes"] == 1
    _check_scores(res, X, pm, w, "logistic", "classifier, pbcd")
    weight = np.bincount(res.fold_, weights=w, minlength=3)
    for p in range(2):
        for f in range(3):
            e = res.estimators_[p][f]
            assert e.sample_weight_sum_ == float(((res.fold_ != f) * w).sum())
            _, _, want, bound = _cells(e, X, pm, w, res.fold_, 3, "logistic")
            if (np.abs(want) > bound * (1 + CLEAR)).all():  # no score can change sides: exact
                tab = restate_group_sums(want[:, None], pm, w, res.fold_, 3, ("sign_error",))
                assert res.test_["sign_error"][p, f] == float(tab[0, 0, f]) / weight[f]
            assert 0 <= res.test_["sign_error"][p, f] <= 1
            # the estimator's own predictions on the held-out rows tell the same story
            out = (res.fold_ == f) & (w > 0)
            miss = (e.predict(X[out]) != labels[out])
            assert abs((w[out] * miss).sum() / weight[f] - res.test_["sign_error"][p, f]) < 1e-12
    assert (res.test_["sign_error"] > 0).any()  # the fits do misclassify some held-out weight


def test_all_subsets():
    from sparsepoly_amd import SparseAllSubsetsRegressor, cross_validate_path

    X, y = _problem(seed=13)
    base = SparseAllSubsetsRegressor(solver="pcd", max_iter=4, tol=0, random_state=0, gamma=1e-3,
                                     beta=1e-3, n_components=4, precision="f32")
    res = _quiet(base.cross_validate_path, X, y, cv=2, gamma=[1e-3, 1e-1])
    assert res.info_ == dict(banks=1, passes=1, members=[4])
    _check_scores(res, X, y, np.ones(N), "squared", "all-subsets")


def test_psgd():
    from sklearn.base import clone

    from sparsepoly_amd import SparseFactorizationMachineRegressor, cross_validate_path

    X, y = _problem(seed=14)
    base = SparseFactorizationMachineRegressor(
        solver="psgd", max_iter=4, tol=-1, n_iter_no_change=100, batch_size=16, eta0=0.05,
        random_state=0, gamma=1e-4, beta=0.1, alpha=1e-2, n_components=4, precision="f32")
    fold = (np.arange(N) % 2).astype(np.int32)
    res = _quiet(cross_validate_path, base, X, y, cv=fold, gamma=[1e-4, 1e-2])
    solo = _quiet(clone(base).set_params(gamma=1e-2).fit, X, y,
                  sample_weight=(fold != 1).astype(np.float64))
    # (psgd sums a minibatch's gradient with atomics, in no fixed order: the tolerance
    # tests/test_hip_weights.py gives two psgd fits of one problem; the scores below are held to
    # each clone's own parameters)
    got = res.estimators_[1][1]
    np.testing.assert_allclose(got.P_, solo.P_, rtol=0, atol=1e-10)
    np.testing.assert_allclose(got.w_, solo.w_, rtol=0, atol=1e-10)
    assert not np.array_equal(got.P_, res.estimators_[1][0].P_)
    _check_scores(res, X, y, np.ones(N), "squared", "psgd")


def test_a_grid_that_varies_fit_linear_takes_two_banks():
    from sparsepoly_amd import SparseFactorizationMachineRegressor, cross_validate_path

    X, y = _problem(seed=15)
    base = SparseFactorizationMachineRegressor(solver="pcd", schedule="colored", max_iter=4, tol=0,
                                               random_state=0, gamma=1e-3, beta=1e-3, alpha=1e-3,
                                               n_components=4, precision="f32")
    res = _quiet(cross_validate_path, base, X, y, cv=2, fit_linear=[True, False],
                 keep_estimators=True)
    assert res.info_ == dict(banks=2, passes=2, members=[2, 2])
    _check_scores(res, X, y, np.ones(N), "squared", "fit_linear grid")
    gone = _quiet(cross_validate_path, base, X, y, cv=2, fit_linear=[True, False],
                  keep_estimators=False)
    assert gone.estimators_ is None
    np.testing.assert_array_equal(gone.test_["loss"], res.test_["loss"])
