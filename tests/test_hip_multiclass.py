"""``sparsepoly_amd.multiclass.OneVsRestClassifier`` and ``fit_concurrently(..., targets=...)`` on
the device.  Needs a real MI355X: ``pytest -m gpu``.

Fits are compared bit for bit: a clone fitted side by side with the others on the shared image
runs the same kernels on the same inputs as its solo fit.  Scores go through the bank, whose bound
``tests/test_hip_bank.py`` derives; a member's own ``decision_function`` sums its components in
another order (a butterfly), within the same count of roundings, hence twice the bank bound between
the two.  ``predict_proba`` is host arithmetic on those scores: a sigmoid has slope at most 1/4,
and dividing by the row's sum s of sigmoids amplifies an error by at most 2 / s, so scores within
the bound (of the order of 1e-13 at these sizes; the test prints it) keep the probabilities within
1e-12 unless every class is rejected with a score far below zero.  scikit-learn's own
``predict_proba`` cannot be called on these members -- theirs returns P(y = +1) as an (n,) vector,
as the reference's does, and the metaestimator indexes ``[:, 1]`` -- so its formula is applied to
the members' own ``decision_function`` here.
"""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.base import clone
from sklearn.multiclass import OneVsRestClassifier as SkOneVsRest

pytestmark = pytest.mark.gpu

CLEAR = 1e-9
N, D_, CLASSES = 200, 40, 4


def _data(seed=0, classes=CLASSES, labels=None):
    rng = np.random.RandomState(seed)
    X = sp.random(N, D_, density=0.2, random_state=rng, data_rvs=rng.randn, format="csr")
    W = rng.randn(D_, classes)
    y = np.asarray((X @ W + 0.1 * rng.randn(N, classes)).argmax(axis=1))
    assert len(np.unique(y)) == classes
    return X, (y if labels is None else np.asarray(labels)[y])


def _base(solver="pcd", loss="squared_hinge", **kw):
    from sparsepoly_amd import SparseFactorizationMachineClassifier

    return SparseFactorizationMachineClassifier(
        degree=2, n_components=4, solver=solver, loss=loss, max_iter=5, random_state=3,
        precision="f64", device=0,
        **{"regularizer": "omegacs" if solver == "pbcd" else "squaredl12", "beta": 1.0,
           "gamma": 1e-3, **kw})


def _fit(est, X, y):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # 5 iterations do not converge
        return est.fit(X, y)


def _same(a, b):
    for name in ("P_", "w_", "lams_"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))


def _bank_bound(ests, X):
    from test_hip_bank import _reference

    return _reference(ests, X)


@pytest.fixture(scope="module", params=["pcd", "pbcd"])
def fitted(request):
    from sparsepoly_amd.multiclass import OneVsRestClassifier

    X, y = _data()
    ovr = _fit(OneVsRestClassifier(_base(request.param, loss="logistic")), X, y)
    yield ovr, X, y
    ovr.release_device()


def test_members_equal_their_solo_fits_and_scikit_learns(fitted):
    """Every member against a plain solo fit of a clone and against scikit-learn's metaestimator
    fitted sequentially, bit for bit; all but the first member trained on the shared image.  (pbcd
    clones are by default fitted one after the other for this: two pbcd fits at a time would give
    each half of the CUs and another order of the partial sums, see the next test.)"""
    ovr, X, y = fitted
    assert (ovr.classes_ == np.arange(CLASSES)).all() and len(ovr.estimators_) == CLASSES
    assert ovr.n_features_in_ == D_
    assert sum(bool(e.shared_image_) for e in ovr.estimators_) == CLASSES - 1
    sk = _fit(SkOneVsRest(clone(ovr.estimator)), X, y)
    for c, est in enumerate(ovr.estimators_):
        solo = _fit(clone(ovr.estimator), X, np.where(y == ovr.classes_[c], 1.0, -1.0))
        _same(est, solo)
        _same(est, sk.estimators_[c])


def test_two_pbcd_fits_at_a_time_equal_solo_fits_with_the_same_share_of_the_cus():
    """``max_concurrent=2`` with pbcd: what ``fit_concurrently`` has always promised for it
    (``tests/test_hip_concurrent.py``).  A fit equals its solo run bit for bit when that run has the
    same share of the CUs; with the whole GPU the persistent pbcd pass has more row groups and adds
    their partial sums in another order (measured here: at most 8.9e-16 apart)."""
    from sparsepoly_amd.engine import co_tenancy
    from sparsepoly_amd.multiclass import OneVsRestClassifier

    X, y = _data()
    ovr = _fit(OneVsRestClassifier(_base("pbcd", loss="logistic"), max_concurrent=2), X, y)
    for c, est in enumerate(ovr.estimators_):
        with co_tenancy(2):
            solo = _fit(clone(ovr.estimator), X, np.where(y == ovr.classes_[c], 1.0, -1.0))
        _same(est, solo)
        whole = _fit(clone(ovr.estimator), X, np.where(y == ovr.classes_[c], 1.0, -1.0))
        np.testing.assert_allclose(est.P_, whole.P_, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(est.w_, whole.w_, rtol=1e-6, atol=1e-9)


def test_decision_function_and_predict(fitted):
    ovr, X, y = fitted
    want, bound, _ = _bank_bound(ovr.estimators_, X)
    # NumPy side first: the exact best and runner-up are clearly apart on every row
    srt = np.sort(want, axis=1)
    assert (srt[:, -1] - srt[:, -2] >= CLEAR * np.abs(want).max()).all()
    sc = ovr.decision_function(X)
    assert sc.shape == (N, CLASSES)
    own = np.stack([e.decision_function(X) for e in ovr.estimators_], axis=1)
    err = np.abs(sc.astype(np.longdouble) - own)
    print("bank against the members' own: largest difference %.3g of twice the bound"
          % float((err / (2 * bound)).max()))
    assert (err <= 2 * bound).all()
    assert (np.abs(sc - want) <= bound).all()
    pred = ovr.predict(X)
    assert (pred == ovr.classes_[sc.argmax(axis=1)]).all()
    sk = SkOneVsRest(clone(ovr.estimator))
    sk.estimators_, sk.classes_ = ovr.estimators_, ovr.classes_
    sk.label_binarizer_ = type("B", (), {"y_type_": "multiclass"})()
    assert (pred == sk.predict(X)).all()
    assert (pred == ovr.classes_[want.argmax(axis=1)]).all()
    assert ovr.score(X, y) == (pred == y).mean()


def test_predict_proba(fitted):
    from sparsepoly_amd import SparseFactorizationMachineClassifier
    from sparsepoly_amd.multiclass import OneVsRestClassifier

    ovr, X, y = fitted
    _, bound, _ = _bank_bound(ovr.estimators_, X)
    print("largest bound of a score: %.3g" % float(bound.max()))
    proba = ovr.predict_proba(X)
    assert proba.shape == (N, CLASSES) and (proba >= 0).all()
    np.testing.assert_allclose(proba.sum(axis=1), 1.0, rtol=0, atol=1e-15 * CLASSES)
    # scikit-learn's formula on the same members' own scores
    Y = np.array([1 / (1 + np.exp(-e.decision_function(X))) for e in ovr.estimators_]).T
    Y /= Y.sum(axis=1)[:, None]
    np.testing.assert_allclose(proba, Y, rtol=0, atol=1e-12)
    hinge = OneVsRestClassifier(SparseFactorizationMachineClassifier(loss="squared_hinge"))
    with pytest.raises(ValueError, match="Probability estimates only available"):
        hinge.predict_proba(X)


def test_two_classes_go_through_one_estimator():
    from sparsepoly_amd.multiclass import OneVsRestClassifier

    X, y = _data(seed=1, classes=2, labels=["no", "yes"])
    ovr = _fit(OneVsRestClassifier(_base(loss="logistic")), X, y)
    plain = _fit(clone(ovr.estimator), X, y)
    assert len(ovr.estimators_) == 1 and list(ovr.classes_) == ["no", "yes"]
    _same(ovr.estimators_[0], plain)
    want, bound, _ = _bank_bound(ovr.estimators_, X)
    assert (np.abs(want) >= CLEAR * np.abs(want).max()).all()  # no exact score at the threshold
    dec = ovr.decision_function(X)
    assert dec.shape == (N,)
    assert (np.abs(dec - plain.decision_function(X)) <= 2 * bound[:, 0]).all()
    assert (ovr.predict(X) == plain.predict(X)).all()
    proba = ovr.predict_proba(X)
    assert proba.shape == (N, 2)
    np.testing.assert_allclose(proba[:, 1], plain.predict_proba(X), rtol=0, atol=1e-12)
    np.testing.assert_allclose(proba.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    ovr.release_device()


def test_string_labels_round_trip():
    from sparsepoly_amd.multiclass import OneVsRestClassifier

    names = ["delta", "alpha", "charlie", "bravo"]
    X, y = _data(seed=2, labels=names)
    ovr = _fit(OneVsRestClassifier(_base()), X, y)
    assert list(ovr.classes_) == sorted(names)
    pred = ovr.predict(X)
    assert pred.dtype == ovr.classes_.dtype and set(pred) <= set(names)
    sc = ovr.decision_function(X)
    assert (pred == ovr.classes_[sc.argmax(axis=1)]).all()
    ovr.release_device()
    assert (ovr.predict(X) == pred).all()  # the bank is rebuilt on use
    ovr.release_device()
    # the same classes as integer codes: the same members, the same predictions
    codes = _fit(OneVsRestClassifier(_base()), X, np.searchsorted(sorted(names), y))
    for a, b in zip(ovr.estimators_, codes.estimators_):
        _same(a, b)
    assert (ovr.classes_[codes.predict(X)] == pred).all()
    codes.release_device()


def test_targets_share_one_image_and_equal_solo_fits():
    from sparsepoly_amd.concurrent import fit_concurrently

    X, y = _data(seed=3)
    targets = [np.where(y == c, 1.0, -1.0) for c in range(CLASSES)]
    ests = [_base() for _ in range(CLASSES)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fitted = fit_concurrently(ests, X, None, targets=targets)
    assert sum(bool(e.shared_image_) for e in fitted) == CLASSES - 1
    for est, t in zip(fitted, targets):
        solo = _fit(_base(), X, t)
        assert not solo.shared_image_
        _same(est, solo)
