"""Per-feature AdaGrad steps, host side (no device): the rule inside the
NumPy restatements against an independent loop over ``restate_pair_gradient``, the untouched
outputs with ``adaptive=None``, the prototypes, and the ``ValueError``s of
``learning_rate='adagrad'`` that need no device.  ``tests/test_hip_pairwise_adagrad.py`` imports
its cases from here."""
import os
import re

import numpy as np
import pytest
from conftest import ROOT
from test_pairwise_host import CASES, GAMMA, HYPER, case_id, pair_params, pair_problem

# the cases of the pairwise device tests that adaptive steps accept (l1 / l21): the three lane
# widths, two orders, fit_linear on and off, the three losses, batch sizes 1, 47 (ragged) and 64
ADAPTIVE_CASES = [c for c in CASES if c["reg"] in ("l1", "l21") and c["precision"] == "f64"
                  and c["n_triples"] == 150]
G0 = 0.01   # of the order of the squares these problems accumulate


def _eta(it):
    """HYPER's rule ('optimal', psgd.py:9-22) written out"""
    e = HYPER["eta0"] * float(it)
    return (HYPER["eta0"] / (1.0 + e * HYPER["beta"]) ** HYPER["power_t"],
            HYPER["eta0"] / (1.0 + e * HYPER["alpha"]) ** HYPER["power_t"])


def plain_loop(case, n_epochs, weights=None):
    """the rule of the issue, feature by feature, over restate_pair_gradient's sums"""
    from sparsepoly_amd.pairwise import restate_pair_gradient

    X, Z, t = pair_problem()
    P, w, lams = pair_params(case)
    P, w = P.copy(), w.copy()
    n_orders, k, d = P.shape
    A_P, A_w = np.zeros((n_orders, d)), np.zeros(d)
    alpha, beta, gamma = HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]]
    it, out = 1, []
    for _ in range(n_epochs):
        sum_loss = 0.0
        for pos in range(0, t.shape[0], case["batch"]):
            tb = t[pos:pos + case["batch"]]
            wb = None if weights is None else weights[pos:pos + case["batch"]]
            val, gP, gw = restate_pair_gradient(P, w, lams, X, Z, tb, case["degree"],
                                                case["loss"], weights=wb)
            sum_loss += val.sum()
            eta_P, eta_w = _eta(it)
            for j in range(d):
                if case["fit_linear"]:
                    g = gw[j] / tb.shape[0]
                    A_w[j] += g * g
                    ew = eta_w / np.sqrt(G0 + A_w[j])
                    w[j] = (w[j] - ew * g) / (1 + ew * alpha)
                for o in range(n_orders):
                    g = gP[o, :, j] / tb.shape[0]
                    A_P[o, j] += g @ g
                    e = eta_P / np.sqrt(G0 + A_P[o, j])
                    p = (P[o, :, j] - e * g) / (1 + e * beta)
                    c = gamma * e / (1 + e * beta)
                    if case["reg"] == "l1":
                        p = np.sign(p) * np.maximum(np.abs(p) - c, 0)
                    elif np.sqrt(p @ p) > c:  # l21.py:43-48 leaves a shorter row as it is
                        p = p * (1 - c / np.sqrt(p @ p))
                    P[o, :, j] = p
            it += 1
        out.append((P.copy(), w.copy(), sum_loss, it, A_P.copy(), A_w.copy()))
    return out


def restated(case, n_epochs, weights=None):
    """[(P, w, sum_loss, it, (A_P, A_w)) after each epoch] by restate_pairwise_epoch"""
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z, t = pair_problem()
    P, w, lams = pair_params(case)
    it, acc, out = 1, None, []
    for _ in range(n_epochs):
        P, w, sl, it, acc = restate_pairwise_epoch(
            P, w, lams, X, Z, t, case["degree"], case["loss"], case["reg"],
            gamma=GAMMA[case["reg"]], batch_size=case["batch"], fit_linear=case["fit_linear"],
            it=it, weights=weights, adaptive=G0, acc=acc, **HYPER)
        out.append((P, w, float(sl), it, acc))
    return (X, Z, t, lams), out


@pytest.mark.parametrize("case", ADAPTIVE_CASES, ids=case_id)
def test_restated_rule_equals_the_plain_loop(case):
    _, got = restated(case, 2)
    want = plain_loop(case, 2)
    for (P, w, sl, it, (A_P, A_w)), (Pw, ww, slw, itw, A_Pw, A_ww) in zip(got, want):
        assert it == itw
        np.testing.assert_allclose(sl, slw, rtol=1e-12)
        np.testing.assert_allclose(P, Pw, rtol=0, atol=1e-13)
        np.testing.assert_allclose(w, ww, rtol=0, atol=1e-13)
        np.testing.assert_allclose(A_P, A_Pw, rtol=1e-12, atol=0)
        np.testing.assert_allclose(A_w, A_ww, rtol=1e-12, atol=0)
    P, w, _, _, (A_P, A_w) = got[-1]
    assert A_P.shape == (P.shape[0], P.shape[2]) and A_w.shape == w.shape
    # the accumulators move the steps: some feature's rate fell to 3/4 of an untouched one's
    assert (G0 + A_P.max()) > (16 / 9) * (G0 + A_P.min())
    if not case["fit_linear"]:
        assert not A_w.any() and np.array_equal(w, pair_params(case)[1])


def test_the_first_step_is_the_constant_rules_with_unit_offset():
    """G0 = 1 and no gradient seen: the rate is eta.  One minibatch whose accumulators are made
    negligible (gradients scaled by weights of 1e-9) equals the plain epoch to that order."""
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    case = ADAPTIVE_CASES[0]
    X, Z, t = pair_problem()
    P, w, lams = pair_params(case)
    kw = dict(gamma=GAMMA["l1"], batch_size=t.shape[0], weights=np.full(t.shape[0], 1e-9),
              alpha=1e-2, beta=0.5, eta0=0.05, learning_rate="constant")
    plain = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, "logistic", "l1", **kw)
    ada = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, "logistic", "l1", adaptive=True, **kw)
    assert len(plain) == 4 and len(ada) == 5 and ada[3] == plain[3] == 2
    np.testing.assert_allclose(ada[0], plain[0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(ada[1], plain[1], rtol=0, atol=1e-15)


def test_accumulators_continue_across_calls_and_are_not_written_through():
    from sparsepoly_amd.pairwise import restate_list_epoch

    from test_pairwise_list_host import CASES as LCASES
    from test_pairwise_list_host import restate_case as list_case

    case = LCASES[0]
    (X, Z, t, P0, w0, lams), _ = list_case(case)
    kw = dict(gamma=GAMMA[case["reg"]], batch_size=case["batch"], adaptive=G0, **HYPER)
    args = (lams, X, Z, t, case["M"], case["degree"], case["objective"], case["loss"], case["reg"])
    P1, w1, _, it1, acc1 = restate_list_epoch(P0, w0, *args, **kw)
    keep = (acc1[0].copy(), acc1[1].copy())
    P2, w2, _, it2, acc2 = restate_list_epoch(P1, w1, *args, it=it1, acc=acc1, **kw)
    assert np.array_equal(acc1[0], keep[0]) and np.array_equal(acc1[1], keep[1])
    assert (acc2[0] >= acc1[0]).all() and (acc2[0] > acc1[0]).any()
    # from zero accumulators the second epoch is another one
    P2z = restate_list_epoch(P1, w1, *args, it=it1, **kw)[0]
    assert np.abs(P2z - P2).max() > 1e-6


def _legacy_pairwise_epoch(P, w, lams, X, Z, triples, degree, loss, regularizer, alpha, beta,
                           gamma, eta0, learning_rate, power_t, batch_size, fit_linear, it):
    """restate_pairwise_epoch as it stood before the adaptive arguments, from the module's own
    unchanged pieces"""
    from sparsepoly_amd import pairwise as pw

    P, w = P.copy(), w.copy()
    sum_loss = np.double(0)
    for pos in range(0, triples.shape[0], batch_size):
        tb = triples[pos:pos + batch_size]
        val, gP, gw = pw.restate_pair_gradient(P, w, lams, X, Z, tb, degree, loss, False, None)
        sum_loss += val.sum()
        eta_P, eta_w = pw._psgd_eta(learning_rate, eta0, alpha, beta, power_t, it)
        if fit_linear:
            w = (w - gw * (eta_w / tb.shape[0])) / (1 + eta_w * alpha)
        P = (P - gP * (eta_P / tb.shape[0])) / (1 + eta_P * beta)
        strength = gamma * eta_P / (1 + eta_P * beta)
        P = np.stack([pw._prox(regularizer, P[o], np.double(strength)) for o in range(P.shape[0])])
        it += 1
    return P, w, sum_loss, it


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], CASES[6]], ids=case_id)
def test_adaptive_none_returns_what_it_returned(case):
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z, t = pair_problem()
    P, w, lams = pair_params(case)
    got = restate_pairwise_epoch(P, w, lams, X, Z, t, case["degree"], case["loss"], case["reg"],
                                 gamma=GAMMA[case["reg"]], batch_size=case["batch"],
                                 fit_linear=case["fit_linear"], adaptive=None, acc=None, **HYPER)
    want = _legacy_pairwise_epoch(P, w, lams, X, Z, t, case["degree"], case["loss"], case["reg"],
                                  HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]], HYPER["eta0"],
                                  HYPER["learning_rate"], HYPER["power_t"], case["batch"],
                                  case["fit_linear"], 1)
    assert len(got) == 4 and got[3] == want[3]
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_list_epoch_with_adaptive_none_is_unchanged_and_adaptive_differs():
    from sparsepoly_amd.pairwise import restate_list_epoch

    from test_pairwise_list_host import CASES as LCASES
    from test_pairwise_list_host import restate_case as list_case

    case = LCASES[1]
    (X, Z, t, P0, w0, lams), ref = list_case(case)
    kw = dict(gamma=GAMMA[case["reg"]], batch_size=case["batch"], fit_linear=case["fit_linear"],
              **HYPER)
    args = (P0, w0, lams, X, Z, t, case["M"], case["degree"], case["objective"], case["loss"],
            case["reg"])
    got = restate_list_epoch(*args, adaptive=None, **kw)
    assert len(got) == 4
    assert np.array_equal(got[0], ref[0][0]) and np.array_equal(got[1], ref[0][1])
    ada = restate_list_epoch(*args, adaptive=G0, **kw)
    assert len(ada) == 5 and ada[3] == got[3] and np.abs(ada[0] - got[0]).max() > 1e-6


def test_restatement_refuses_what_the_engine_refuses():
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z, t = pair_problem()
    P, w, lams = pair_params(CASES[2])
    for reg in ("squaredl12", "squaredl21"):
        with pytest.raises(ValueError, match="adaptive steps cannot be combined"):
            restate_pairwise_epoch(P, w, lams, X, Z, t, 3, "logistic", reg, adaptive=True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive and finite"):
            restate_pairwise_epoch(P, w, lams, X, Z, t, 3, "logistic", "l1", adaptive=bad)


def test_estimator_value_errors_need_no_device(monkeypatch):
    """learning_rate='adagrad' with a squared norm, a plug-in regularizer or distributed=True is
    refused before a handle exists; G0 is a class attribute, not a constructor keyword"""
    import scipy.sparse as sp

    from sparsepoly_amd import (SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRanker,
                                SparseFactorizationMachineRegressor)
    from sparsepoly_amd import engine as engine_mod
    from sparsepoly_amd import regularizer as R

    def no_device(*a, **k):
        raise AssertionError("a device handle was requested")

    monkeypatch.setattr(engine_mod.HipEngine, "__init__", no_device)
    rng = np.random.RandomState(0)
    Xs = sp.csr_matrix(rng.randn(12, 5))
    y = rng.randn(12)
    kw = dict(solver="psgd", learning_rate="adagrad", max_iter=1)
    for cls, yy in ((SparseFactorizationMachineRegressor, y),
                    (SparseFactorizationMachineClassifier, np.sign(y))):
        assert "adagrad_init" not in cls().get_params() and cls.adagrad_init == 1.0
        for reg in ("squaredl12", "squaredl21"):
            with pytest.raises(ValueError, match="squaredl12 / squaredl21"):
                cls(regularizer=reg, **kw).fit(Xs, yy)
        with pytest.raises(ValueError, match="one GPU"):
            cls(regularizer="l1", distributed=True, **kw).fit(Xs, yy)
        est = cls(regularizer="l21", **kw)
        with pytest.raises(AssertionError, match="a device handle was requested"):
            est.fit(Xs, yy)     # accepted: the next thing it needs is the device
        assert not hasattr(est, "adagrad_P_")

    class Plugin(R.L1):
        pass

    class Est(SparseFactorizationMachineRegressor):  # a registry with a user's regularizer
        _REGULARIZERS = dict(SparseFactorizationMachineRegressor._REGULARIZERS, mine=Plugin)

    with pytest.raises(ValueError, match="built-in regularizers"):
        Est(regularizer="mine", **kw).fit(Xs, y)
    # any other solver ignores learning_rate as before
    with pytest.raises(AssertionError, match="a device handle was requested"):
        SparseFactorizationMachineRegressor(solver="pcd", learning_rate="adagrad",
                                            regularizer="squaredl12", max_iter=1).fit(Xs, y)
    X, Z, t = pair_problem()
    for reg in ("squaredl12", "squaredl21"):
        with pytest.raises(ValueError, match="squaredl12 / squaredl21"):
            SparseFactorizationMachineRanker(regularizer=reg, learning_rate="adagrad").fit(
                X, Z, triples=t)
    with pytest.raises(ValueError, match="learning_rate adagrads is not supported"):
        SparseFactorizationMachineRanker(regularizer="l1", learning_rate="adagrads").fit(
            X, Z, triples=t)


def test_extend_features_pads_the_accumulators():
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    est = SparseFactorizationMachineRegressor(degree=2, n_components=3, solver="psgd",
                                              regularizer="l1", learning_rate="adagrad")
    rng = np.random.RandomState(0)
    est.P_, est.w_, est.lams_ = rng.randn(1, 3, 6), rng.randn(6), np.ones(3)
    est.adagrad_P_, est.adagrad_w_ = rng.rand(1, 6), rng.rand(6)
    aP, aw = est.adagrad_P_.copy(), est.adagrad_w_.copy()
    new = est.extend_features(2)
    assert list(new) == [6, 7]
    assert est.adagrad_P_.shape == (1, 8) and est.adagrad_w_.shape == (8,)
    assert np.array_equal(est.adagrad_P_[:, :6], aP) and not est.adagrad_P_[:, 6:].any()
    assert np.array_equal(est.adagrad_w_[:6], aw) and not est.adagrad_w_[6:].any()
    assert est.P_.shape == (1, 3, 8)


def test_header_capi_and_library_agree_on_the_adaptive_symbols():
    from sparsepoly_amd import _capi

    with open(os.path.join(ROOT, "include", "spfm.h")) as f:
        header = f.read()
    for name in ("spfm_psgd_set_adaptive", "spfm_psgd_get_adaptive"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS
    assert _capi.LEARNING_RATE == {"constant": 0, "optimal": 1, "pegasos": 2, "invscaling": 3}
