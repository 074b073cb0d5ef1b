"""Full-catalogue softmax of the ranking fit on the device against the
NumPy restatement; problem and cases from ``tests/test_pairwise_full_host.py``, tolerances from
``tests/test_hip_pairwise_inbatch.py`` (the same matrix instruction, atomics and prox step)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
from test_pairwise_full_host import (CASES, N_CAND, N_CTX, case_id, full_params, full_problem,
                                     restate_case)
from test_pairwise_host import GAMMA, HYPER

pytestmark = pytest.mark.gpu

P_ATOL = {"f64": 1e-9, "f32": 5e-5}
SL_RTOL = {"f64": 1e-10, "f32": 1e-5}


def _engine(case, opts=(), comm=False, sampler=True):
    from sparsepoly_amd.engine import HipEngine

    X, Z, pairs, I, _ = full_problem()
    P0, w0, lams = full_params(case)
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    eng = HipEngine(0, case["precision"])
    for key, val in opts:
        eng.set_option(key, val)
    if comm:
        eng.comm_init(HipEngine.comm_unique_id(), 1, 0)
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0.copy(), w0.copy(), lams)
    eng.configure("psgd", "logistic", case["reg"], case["degree"])
    if sampler:
        eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I, restate_case(case)[0])
    return eng, (pairs + np.array([0, N_CTX])).astype(np.int32)


def _step(case, batch=None):
    return (case["degree"], HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]], HYPER["eta0"],
            HYPER["learning_rate"], HYPER["power_t"], case["batch"] if batch is None else batch)


def _close(case, P, w, Pr, wr):
    np.testing.assert_allclose(P, Pr, rtol=0, atol=P_ATOL[case["precision"]])
    np.testing.assert_allclose(w, wr, rtol=0, atol=P_ATOL[case["precision"]])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_eval_then_one_epoch_against_the_restatement(case):
    """the eval gives the rows' losses whatever the batch and keeps the parameters' bits"""
    from sparsepoly_amd.pairwise import restate_full_gradient

    F, ((Pr, wr, slr, itr),) = restate_case(case)
    want = restate_full_gradient(*full_params(case), *full_problem()[:3], F,
                                 case["degree"])[0].sum()
    eng, ps = _engine(case)
    try:
        before = eng.get_params()
        sls = [eng.psgd_full_eval(case["degree"], batch, ps) for batch in (case["batch"], 1)]
        np.testing.assert_allclose(sls, want, rtol=SL_RTOL[case["precision"]])
        np.testing.assert_allclose(sls[1], sls[0], rtol=SL_RTOL[case["precision"]])
        assert all(np.array_equal(a, b) for a, b in zip(before, eng.get_params()))
        sl, it = eng.psgd_full_epoch(*_step(case), ps, case["fit_linear"], 1)
        assert it == itr
        np.testing.assert_allclose(sl, slr, rtol=SL_RTOL[case["precision"]])
        P, w = eng.get_params()
        _close(case, P, w, Pr, wr)
        assert np.abs(P - full_params(case)[0]).max() > 1e-4     # it did train
    finally:
        eng.close()


def test_graph_replay_agrees_with_eager_launches():
    """batch 2: 35 minibatches, one replayed run of 32 and 3 single table-driven launches"""
    case = CASES[0]
    ref = restate_case(case, 2, 3)[1]
    for opts in ((), (("psgd_eager", 1),)):
        eng, ps = _engine(case, opts)
        try:
            it = 1
            for ep in range(3):
                sl, it = eng.psgd_full_epoch(*_step(case, 2), ps, case["fit_linear"], it)
                np.testing.assert_allclose(sl, ref[ep][2], rtol=SL_RTOL["f64"])
                _close(case, *eng.get_params(), ref[ep][0], ref[ep][1])
            assert it == ref[2][3] == 1 + 3 * 35
        finally:
            eng.close()


def _codes(eng, ps, batch=8):
    pp = ps.ctypes.data_as(C.POINTER(C.c_int32))
    itc, sl = C.c_int64(1), C.c_double()
    ep = eng._lib.spfm_psgd_full_epoch(eng._h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, batch, pp,
                                       ps.shape[0], 1, C.byref(itc), C.byref(sl))
    ev = eng._lib.spfm_psgd_full_eval(eng._h, 2, batch, pp, ps.shape[0], C.byref(sl))
    assert itc.value == 1
    return ep, ev


@pytest.mark.parametrize("how,code", [
    ("no_sampler", "SPFM_ERR_INVALID"), ("not_a_positive", "SPFM_ERR_INVALID"),
    ("candidate_outside", "SPFM_ERR_INVALID"), ("comm", "SPFM_ERR_UNSUPPORTED"),
    ("pairs_det", "SPFM_ERR_UNSUPPORTED"), ("weighted", "SPFM_ERR_UNSUPPORTED")])
def test_refusals_leave_the_parameters_bit_for_bit(how, code):
    from sparsepoly_amd import _capi

    eng, ps = _engine(CASES[0], comm=how == "comm", sampler=how != "no_sampler")
    try:
        before = eng.get_params()
        ps = ps.copy()
        if how == "not_a_positive":    # context 2's one negative, candidate 150
            ps[0] = (2, N_CTX + 150)
        if how == "candidate_outside":
            ps[0, 1] = N_CTX + N_CAND
        if how == "pairs_det":
            eng.psgd_pairs_set_deterministic(1)
        if how == "weighted":
            eng.set_sample_weight(np.ones(N_CTX + N_CAND))
        assert _codes(eng, ps) == (getattr(_capi, code),) * 2
        assert all(np.array_equal(a, b) for a, b in zip(before, eng.get_params()))
    finally:
        eng.close()


def test_estimator_fit_and_full_softmax_loss_against_the_rebuilt_loop():
    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import (_forbidden, _prepare_pairs, epoch_pairs,
                                         restate_full_epoch, restate_full_gradient)

    X, Z, _, I, E = full_problem()
    est = SparseFactorizationMachineRanker(
        degree=2, n_components=8, regularizer="l1", alpha=1e-2, beta=0.5, gamma=0.003, eta0=0.05,
        max_iter=2, tol=-1e9, shuffle=True, batch_size=32, learning_rate="adagrad",
        random_state=7, precision="f64").fit(X, Z, interactions=I, sampler="full",
                                             objective="softmax", exclude=E)
    rng = np.random.RandomState(7)   # the estimator's draws from the same seed
    Xa, Za = _prepare_pairs(est, X, Z)
    Ic, F = _forbidden(I, E, N_CTX, N_CAND)
    P = 0.01 * rng.randn(1, 8, Xa.shape[1])
    w, lams = np.zeros(Xa.shape[1]), np.ones(8)
    pos = np.stack([np.repeat(np.arange(N_CTX), np.diff(Ic.indptr)), Ic.indices], axis=1)
    it, acc = 1, None
    for pr in epoch_pairs(rng, 2, pos, True):
        P, w, _, it, acc = restate_full_epoch(
            P, w, lams, Xa, Za, pr, F, 2, "l1", 1e-2, 0.5, 0.003, 0.05, est._base_rate(), 1.0, 32,
            True, it, adaptive=True, acc=acc)
    assert est.it_ == it
    np.testing.assert_allclose(est.P_, P, rtol=0, atol=1e-9)
    np.testing.assert_allclose(est.w_, w, rtol=0, atol=1e-9)
    want = restate_full_gradient(P, w, lams, Xa, Za, pos, F, 2)[0].mean()
    np.testing.assert_allclose(est.full_softmax_loss(X, Z, I, E, 50), want, rtol=1e-10)
