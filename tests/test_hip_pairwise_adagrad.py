"""Per-feature AdaGrad steps behind the pair, weighted-pair and list
gradients on the device, against the NumPy restatements with ``adaptive=...``, and one ranker fit
with ``learning_rate='adagrad'``.  Needs a real MI355X: ``pytest -m gpu``.  The problems and cases
are those of ``tests/test_pairwise_host.py`` / ``tests/test_pairwise_list_host.py``; the
restatement's rule is checked on the host in ``tests/test_pairwise_adagrad_host.py``.

Tolerances are the psgd bars of ``tests/test_hip_pairwise.py``: P, w and the accumulators to 1e-9
(f64 handle), sum_loss to 1e-10 relative, ``it`` exactly."""
import warnings

import numpy as np
import pytest
from test_hip_pairwise import P_ATOL, SL_RTOL, _stacked
from test_pairwise_adagrad_host import ADAPTIVE_CASES, G0, restated
from test_pairwise_host import GAMMA, HYPER, case_id, pair_params

pytestmark = pytest.mark.gpu


def _engine(X, Z, P0, w0, lams, case):
    from sparsepoly_amd.engine import HipEngine

    S, _ = _stacked(X, Z, np.zeros((0, 3), dtype=np.int32))
    eng = HipEngine(0, "f64")
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0.copy(), w0.copy(), lams)
    eng.configure("psgd", case["loss"], case["reg"], case["degree"])
    eng.psgd_set_adaptive(1, G0)
    return eng


def _step(case):
    return (case["degree"], HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]], HYPER["eta0"],
            HYPER["learning_rate"], HYPER["power_t"], case["batch"])


def _compare(eng, ep, sl, it, ref):
    P, w = eng.get_params()
    aP, aw = eng.psgd_get_adaptive()
    Pr, wr, slr, itr, (aPr, awr) = ref
    print("epoch %d: max|dP| = %.3e  max|dw| = %.3e  max|dA| = %.3e  rel dloss = %.3e"
          % (ep + 1, np.abs(P - Pr).max(), np.abs(w - wr).max(), np.abs(aP - aPr).max(),
             abs(sl - slr) / abs(slr)))
    assert it == itr
    np.testing.assert_allclose(sl, slr, rtol=SL_RTOL["f64"])
    np.testing.assert_allclose(P, Pr, rtol=0, atol=P_ATOL["f64"])
    np.testing.assert_allclose(w, wr, rtol=0, atol=P_ATOL["f64"])
    np.testing.assert_allclose(aP, aPr, rtol=0, atol=P_ATOL["f64"])
    np.testing.assert_allclose(aw, awr, rtol=0, atol=P_ATOL["f64"])
    return P


@pytest.mark.parametrize("case", ADAPTIVE_CASES, ids=case_id)
def test_pair_epochs_against_the_restatement(case):
    (X, Z, t, lams), ref = restated(case, 2)
    _, ts = _stacked(X, Z, t)
    P0, w0, _ = pair_params(case)
    eng = _engine(X, Z, P0, w0, lams, case)
    it = 1
    try:
        for ep in range(2):
            sl, it = eng.psgd_pairs_epoch(*_step(case), ts, case["fit_linear"], it)
            P = _compare(eng, ep, sl, it, ref[ep])
        assert np.abs(P - P0).max() > 1e-4     # it did train
    finally:
        eng.close()


@pytest.mark.parametrize("case", [ADAPTIVE_CASES[0], ADAPTIVE_CASES[1]], ids=case_id)
def test_weighted_pair_epochs_against_the_restatement(case):
    wt = np.random.RandomState(11).uniform(0.0, 2.0, 150)
    wt[::7] = 0.0
    (X, Z, t, lams), ref = restated(case, 2, weights=wt)
    _, ts = _stacked(X, Z, t)
    P0, w0, _ = pair_params(case)
    eng = _engine(X, Z, P0, w0, lams, case)
    it = 1
    try:
        for ep in range(2):
            sl, it = eng.psgd_pairs_epoch_weighted(*_step(case), ts, wt, case["fit_linear"], it)
            _compare(eng, ep, sl, it, ref[ep])
    finally:
        eng.close()


@pytest.mark.parametrize("ci", [0, 1], ids=["softmax", "list"])
def test_list_epochs_against_the_restatement(ci):
    from sparsepoly_amd.pairwise import restate_list_epoch

    from test_pairwise_list_host import CASES as LCASES
    from test_pairwise_list_host import restate_case as list_case

    case = LCASES[ci]
    assert case["objective"] == ("softmax", "list")[ci] and case["precision"] == "f64"
    (X, Z, t, P0, w0, lams), _ = list_case(case)
    _, ts = _stacked(X, Z, t)
    eng = _engine(X, Z, P0, w0, lams, case)
    P, w, it_r, acc = P0, w0, 1, None
    it = 1
    try:
        for ep in range(2):
            P, w, slr, it_r, acc = restate_list_epoch(
                P, w, lams, X, Z, t, case["M"], case["degree"], case["objective"], case["loss"],
                case["reg"], gamma=GAMMA[case["reg"]], batch_size=case["batch"],
                fit_linear=case["fit_linear"], it=it_r, adaptive=G0, acc=acc, **HYPER)
            sl, it = eng.psgd_lists_epoch(*_step(case), ts, case["M"], case["objective"],
                                          case["fit_linear"], it)
            _compare(eng, ep, sl, it, (P, w, float(slr), it_r, acc))
    finally:
        eng.close()


E2E_EPOCHS = 3
E2E_KW = dict(degree=2, n_components=6, fit_lower=None, fit_linear=True, regularizer="l1",
              alpha=1e-3, beta=1e-2, gamma=1e-4, eta0=0.1, learning_rate="adagrad",
              batch_size=64, max_iter=E2E_EPOCHS, tol=-1.0, n_iter_no_change=1000, shuffle=True,
              random_state=3, precision="f64")


def test_ranker_fit_with_adagrad_and_the_uniform_sampler():
    """the fit against the loop rebuilt from restate_sample (the uniform device sampler is exact:
    tests/test_hip_pairwise_sample.py) and restate_pairwise_epoch(adaptive=...) under the same
    random_state; then a warm start continues it_ and the accumulators"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import restate_pairwise_epoch, restate_sample
    from test_hip_pairwise import planted_problem

    X, Z, train, _ = planted_problem()
    d = X.shape[1]
    est = SparseFactorizationMachineRanker(**E2E_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=train, n_negatives=2, resample=True, sampler="uniform")
    rng = check_random_state(E2E_KW["random_state"])
    P, w, lams = 0.01 * rng.randn(1, 6, d), np.zeros(d), np.ones(6)
    P_init = P.copy()
    seed = rng.randint(0, 2 ** 31 - 1)
    m = train.nnz * 2
    it, acc, losses = 1, None, []
    for ep in range(E2E_EPOCHS):
        order = rng.permutation(m)
        t, _, _ = restate_sample(P, w, lams, X, Z, train, 2, 2, 1, 64, seed, ep, order=order)
        P, w, sl, it, acc = restate_pairwise_epoch(
            P, w, lams, X, Z, t, 2, "logistic", "l1", 1e-3, 1e-2, 1e-4, 0.1, "constant", 1.0, 64,
            True, it, adaptive=SparseFactorizationMachineRanker.adagrad_init, acc=acc)
        losses.append(float(sl) / m)
    assert est.it_ == it == 1 + E2E_EPOCHS * 25 and est.n_iter_ == E2E_EPOCHS - 1
    print("max|dP| = %.3e, max|dw| = %.3e, max|dA| = %.3e, losses %s"
          % (np.abs(est.P_ - P).max(), np.abs(est.w_ - w).max(),
             np.abs(est.adagrad_P_ - acc[0]).max(), losses))
    np.testing.assert_allclose(est.P_, P, rtol=0, atol=1e-9 * E2E_EPOCHS)
    np.testing.assert_allclose(est.w_, w, rtol=0, atol=1e-9 * E2E_EPOCHS)
    np.testing.assert_allclose(est.adagrad_P_, acc[0], rtol=0, atol=1e-9 * E2E_EPOCHS)
    np.testing.assert_allclose(est.adagrad_w_, acc[1], rtol=0, atol=1e-9 * E2E_EPOCHS)
    assert est.adagrad_P_.shape == (1, d) and est.adagrad_w_.shape == (d,)
    assert losses[-1] < losses[0] and np.abs(P - P_init).max() > 1e-3
    # a second fit with warm_start continues it_ and grows the accumulators
    before = est.adagrad_P_.copy()
    est.set_params(warm_start=True, max_iter=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=train, n_negatives=2, sampler="uniform")
    assert est.it_ == it + 25
    assert (est.adagrad_P_ >= before).all() and (est.adagrad_P_ > before).any()
