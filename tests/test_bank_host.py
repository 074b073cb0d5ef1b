"""``sparsepoly_amd.bank`` and ``sparsepoly_amd.multiclass`` without a device: the NumPy
restatement ``restate_bank_scores`` against reference-produced predictions, its independence of
the bank's composition, the argument errors that are raised before any device use, the C
boundary's declarations, and the metaestimator's scikit-learn protocol."""
import os
import pickle
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import load_golden
from sklearn.base import clone
from sklearn.utils.validation import NotFittedError
from test_explain_host import rows_matrix
from test_ranking_host import all_subsets, fm

from sparsepoly_amd.bank import ModelBank, restate_bank_scores
from sparsepoly_amd.multiclass import OneVsRestClassifier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_device(monkeypatch):
    from sparsepoly_amd import engine

    def no_device(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", no_device)


def _golden_model(z, tag):
    """the estimator ``test_ranking_host.py`` builds for ``tag`` and its recorded predictions"""
    X = z["X"]
    if "|" in tag:
        deg, fl = tag.split("|")
        est = fm(int(deg[3:]), 4, X.shape[1], fit_lower=None if fl == "None" else fl)
        est.P_, est.w_, est.lams_ = z["est_P|" + tag], z["est_w|" + tag], z["lams"]
        return est, z["est_pred|" + tag]
    est = fm(int(tag[3:]), 4, X.shape[1], fit_lower=None, fit_linear=False)
    est.P_, est.w_, est.lams_ = z["P"][None], np.zeros(X.shape[1]), z["lams"]
    return est, z["pred|" + tag]


@pytest.mark.parametrize("tag", ["deg2", "deg3", "deg4", "deg5", "deg2|explicit", "deg3|explicit",
                                 "deg3|None"])
def test_restatement_reproduces_the_recorded_predictions(tag):
    """a bank [recorded model, another model of its kind with 7 components, recorded model]: the
    first and the last column are the recorded predictions of g6_anova.npz, at the tolerance
    ``test_ranking_host.py`` uses for ``restate_scores``"""
    z = load_golden("g6_anova.npz")
    est, want = _golden_model(z, tag)
    other = fm(est.degree, 7, z["X"].shape[1], fit_lower=est.fit_lower, fit_linear=est.fit_linear,
               seed=3)
    got = restate_bank_scores([est, other, est], z["X"])
    assert got.shape == (z["X"].shape[0], 3)
    for c in (0, 2):
        np.testing.assert_allclose(got[:, c], want, rtol=0, atol=1e-10)
    assert np.abs(got[:, 1] - want).max() > 1e-3


@pytest.mark.parametrize("wide", [False, True])
def test_a_column_does_not_depend_on_the_other_members(wide):
    X = rows_matrix([0, 1, 4, 9, 12, 0], 12, seed=1)
    for ests in ([fm(3, k, 12, "explicit", True, seed=k) for k in (1, 5, 3)],
                 [fm(4, k, 12, "augment", False, seed=k) for k in (2, 6, 3)],
                 [all_subsets(k, 12, seed=k) for k in (3, 1, 4)]):
        full = restate_bank_scores(ests, X, wide=wide)
        assert full.dtype == (np.longdouble if wide else np.double)
        for f, est in enumerate(ests):
            assert (restate_bank_scores([est], X, wide=wide)[:, 0] == full[:, f]).all()
        back = restate_bank_scores(ests[::-1], X, wide=wide)
        assert (back[:, ::-1] == full).all()


def test_bank_argument_errors_come_before_any_device_use(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRegressor, _capi

    _no_device(monkeypatch)
    X = rows_matrix([0, 2, 3], 10)
    a = fm(3, 3, 10, "explicit", True)
    for call in (ModelBank, lambda e: restate_bank_scores(e, X)):
        with pytest.raises(ValueError, match="at least one"):
            call([])
        with pytest.raises(NotFittedError):
            call([a, SparseFactorizationMachineRegressor()])
        for other, what in ((fm(2, 3, 10, "explicit", True), "degree"),
                            (fm(3, 3, 10, None, True), "fit_lower|block"),
                            (fm(3, 3, 10, "explicit", False), "fit_linear"),
                            (fm(3, 3, 11, "explicit", True), "features")):
            with pytest.raises(ValueError, match="disagrees with member 0 on .*(%s)" % what):
                call([a, other])
        with pytest.raises(ValueError, match="all-subsets"):
            call([a, all_subsets(3, 10)])
        with pytest.raises(ValueError, match="all-subsets"):
            call([all_subsets(3, 10), a])
        too_many = [fm(2, 1, 10)] * (_capi.BANK_MAX_MODELS + 1)
        with pytest.raises(ValueError, match="SPFM_BANK_MAX_MODELS"):
            call(too_many)
        too_wide = [fm(2, _capi.BANK_MAX_COMPONENTS // 4 + 1, 4)] * 4
        with pytest.raises(ValueError, match="SPFM_BANK_MAX_COMPONENTS"):
            call(too_wide)
    with pytest.raises(ValueError, match="precision"):
        ModelBank([a], precision="f16")
    with pytest.raises(ValueError, match="features"):
        restate_bank_scores([a], X[:, :9])
    # reaching the device is the only thing left to go wrong for good arguments
    with pytest.raises(AssertionError, match="device handle"):
        ModelBank([a, fm(3, 5, 10, "explicit", True)])
    # 64 models of 30 components are within the caps
    assert 64 <= _capi.BANK_MAX_MODELS and 64 * 30 <= _capi.BANK_MAX_COMPONENTS


def test_one_vs_rest_fit_argument_errors_come_before_any_device_use(monkeypatch):
    from sparsepoly_amd import (SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)

    _no_device(monkeypatch)
    X = rows_matrix([2, 2, 3, 1, 2, 3], 10)
    ovr = OneVsRestClassifier(SparseFactorizationMachineClassifier(n_components=2))
    y = np.array([0, 1, 2, 0, 1, 2])
    with pytest.raises(TypeError, match="multilabel and 2-d"):
        ovr.fit(X, np.eye(3)[y])  # an indicator matrix
    with pytest.raises(TypeError, match="multilabel and 2-d"):
        ovr.fit(X, y[:, None])
    with pytest.raises(TypeError, match="multilabel and 2-d"):
        ovr.fit(X, y + 0.5)  # a continuous target
    with pytest.raises(ValueError, match="entries"):
        ovr.fit(X, y[:-1])
    with pytest.raises(ValueError, match="single class"):
        ovr.fit(X, np.zeros(6, dtype=int))
    with pytest.raises(TypeError, match="estimator must be"):
        OneVsRestClassifier(SparseFactorizationMachineRegressor()).fit(X, y)
    with pytest.raises(ValueError, match="max_concurrent"):
        OneVsRestClassifier(ovr.estimator, max_concurrent=0).fit(X, y)
    for name in ("decision_function", "predict"):
        with pytest.raises(NotFittedError):
            getattr(ovr, name)(X)
    hinge = OneVsRestClassifier(SparseFactorizationMachineClassifier(loss="squared_hinge"))
    with pytest.raises(ValueError, match="Probability estimates only available"):
        hinge.predict_proba(X)
    assert not hasattr(ovr, "estimators_")


def test_header_capi_and_library_agree_on_the_new_symbols():
    from sparsepoly_amd import _capi

    names = ("spfm_bank_set", "spfm_bank_scores", "spfm_bank_argmax", "spfm_bank_losses",
             "spfm_bank_mean", "spfm_bank_set_partition", "spfm_bank_info", "spfm_bank_release")
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS
    assert re.search(r"#define SPFM_BANK_MAX_MODELS %d\b" % _capi.BANK_MAX_MODELS, header)
    assert re.search(r"#define SPFM_BANK_MAX_COMPONENTS %d\b" % _capi.BANK_MAX_COMPONENTS, header)
    lib = _capi.load()
    for name in names:
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name


def test_one_vs_rest_follows_the_estimator_protocol():
    from sparsepoly_amd import SparseAllSubsetsClassifier, SparseFactorizationMachineClassifier

    base = SparseFactorizationMachineClassifier(degree=3, n_components=5, loss="logistic")
    ovr = OneVsRestClassifier(base, max_concurrent=2)
    twin = clone(ovr)
    assert twin is not ovr and twin.estimator is not base
    assert twin.get_params()["estimator__degree"] == 3 and twin.max_concurrent == 2
    assert twin.get_params(deep=False).keys() == {"estimator", "max_concurrent", "devices"}
    twin.set_params(estimator__n_components=7, devices=[0])
    assert twin.estimator.n_components == 7 and twin.devices == [0] and base.n_components == 5
    twin.set_params(estimator=SparseAllSubsetsClassifier())
    assert isinstance(twin.estimator, SparseAllSubsetsClassifier)
    # a fitted metaestimator pickles without its device state
    ovr.estimators_ = [fm(3, 5, 6, cls=SparseFactorizationMachineClassifier, seed=c)
                       for c in range(3)]
    ovr.classes_ = np.array(["a", "b", "c"])

    class Handle(object):
        def close(self):
            self.closed = True

        def __reduce__(self):
            raise TypeError("a device handle cannot be pickled")

    handle = ovr._device_bank = Handle()
    back = pickle.loads(pickle.dumps(ovr))
    assert getattr(back, "_device_bank", None) is None
    assert (back.classes_ == ovr.classes_).all() and len(back.estimators_) == 3
    assert (back.estimators_[1].P_ == ovr.estimators_[1].P_).all()
    ovr.release_device()
    assert handle.closed and ovr._device_bank is None


def test_targets_with_a_list_of_matrices_is_refused(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.concurrent import fit_concurrently

    _no_device(monkeypatch)
    X = sp.csr_matrix(np.eye(4))
    y = np.arange(4.0)
    ests = [SparseFactorizationMachineRegressor(), SparseFactorizationMachineRegressor()]
    with pytest.raises(ValueError, match="targets="):
        fit_concurrently(ests, [X, X], [y, y], targets=[y, y])
    with pytest.raises(ValueError, match="one entry per estimator"):
        fit_concurrently(ests, X, None, targets=[y])
    with pytest.raises(TypeError):
        fit_concurrently(ests, X, None, None, None, True, [y, y])  # keyword only
