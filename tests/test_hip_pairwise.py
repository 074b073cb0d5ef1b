"""Pairwise ranking fit on the device against the NumPy restatement of
``sparsepoly_amd/pairwise.py``.  Needs a real MI355X: ``pytest -m gpu``.  The problem and the
cases come from ``tests/test_pairwise_host.py``, which also shows that every restated margin
used here is clear of zero.

Tolerances are the project's own bars for this solver (tests/test_hip_psgd.py): the gradient
scatter uses hardware f64 atomics, so the summation order inside a minibatch is not fixed, and
nothing else differs -- P and w to 1e-9 (f64 handle) / 5e-5 (f32), sum_loss to 1e-10 / 1e-5
relative, ``it`` exactly."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from test_pairwise_host import (CASES, D_CTX, GAMMA, HYPER, N_CTX, case_id, pair_params,
                                pair_problem, restate_case)

pytestmark = pytest.mark.gpu

P_ATOL = {"f64": 1e-9, "f32": 5e-5}
SL_RTOL = {"f64": 1e-10, "f32": 1e-5}


def _stacked(X, Z, t):
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    return S, (t + np.array([0, X.shape[0], X.shape[0]])).astype(np.int32)


def _engine(case, X, Z, opts=()):
    from sparsepoly_amd.engine import HipEngine

    S, _ = _stacked(X, Z, np.zeros((0, 3), dtype=np.int32))
    P0, w0, lams = pair_params(case)
    eng = HipEngine(0, case["precision"])
    for key, val in opts:
        eng.set_option(key, val)
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", case["loss"], case["reg"], case["degree"])
    return eng


def _epoch(eng, case, ts, it):
    return eng.psgd_pairs_epoch(case["degree"], HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]],
                                HYPER["eta0"], HYPER["learning_rate"], HYPER["power_t"],
                                case["batch"], ts, case["fit_linear"], it)


# ------------------------------------------------------------------ 1. epochs vs the restatement
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_and_two_epochs_against_the_restatement(case):
    (X, Z, t, lams), ref = restate_case(case, 2)
    _, ts = _stacked(X, Z, t)
    eng = _engine(case, X, Z)
    prec = case["precision"]
    it = 1
    try:
        for ep in range(2):
            sl, it = _epoch(eng, case, ts, it)
            P, w = eng.get_params()
            Pr, wr, slr, itr = ref[ep]
            print("epoch %d: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
                  % (ep + 1, np.abs(P - Pr).max(), np.abs(w - wr).max(), abs(sl - slr) / abs(slr)))
            assert it == itr
            np.testing.assert_allclose(sl, slr, rtol=SL_RTOL[prec])
            np.testing.assert_allclose(P, Pr, rtol=0, atol=P_ATOL[prec])
            np.testing.assert_allclose(w, wr, rtol=0, atol=P_ATOL[prec])
        assert np.abs(P - pair_params(case)[0]).max() > 1e-4     # it did train
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. graph replay vs eager
@pytest.mark.parametrize("reg", ["l1", "squaredl12"])
def test_graph_replay_agrees_with_eager_launches(reg):
    """38 minibatches per epoch: one replayed run of 32 and 6 single launches.  The squared-norm
    prox replays from its second (warm) epoch on."""
    case = dict(CASES[1], reg=reg, batch=4)
    (X, Z, t, lams), ref = restate_case(case, 3)
    _, ts = _stacked(X, Z, t)
    res = {}
    for mode, opts in (("graph", ()), ("eager", (("psgd_eager", 1),))):
        eng = _engine(case, X, Z, opts)
        it, sls = 1, []
        for _ in range(3):
            sl, it = _epoch(eng, case, ts, it)
            sls.append(sl)
        res[mode] = (eng.get_params(), np.array(sls), it, eng.get_option("psgd_redone"))
        eng.close()
    print("psgd_redone: graph %d, eager %d" % (res["graph"][3], res["eager"][3]))
    assert res["eager"][3] == 0
    for mode in res:
        (P, w), sls, it, _ = res[mode]
        assert it == ref[2][3] == 1 + 3 * 38
        np.testing.assert_allclose(sls, [r[2] for r in ref], rtol=1e-10, err_msg=mode)
        np.testing.assert_allclose(P, ref[2][0], rtol=0, atol=1e-9, err_msg=mode)
        np.testing.assert_allclose(w, ref[2][1], rtol=0, atol=1e-9, err_msg=mode)
    np.testing.assert_allclose(res["graph"][0][0], res["eager"][0][0], rtol=0, atol=1e-9)


# ------------------------------------------------------------------ 3. context linear weights
def test_context_linear_weights_get_no_gradient():
    from sparsepoly_amd.pairwise import _psgd_eta

    case = CASES[1]
    X, Z, t = pair_problem()
    _, ts = _stacked(X, Z, t)
    w0 = pair_params(case)[1]
    for alpha in (0.0, 1e-2):
        eng = _engine(case, X, Z)
        it = 1
        for _ in range(3):
            _, it = eng.psgd_pairs_epoch(case["degree"], alpha, HYPER["beta"], GAMMA[case["reg"]],
                                         HYPER["eta0"], "optimal", HYPER["power_t"], case["batch"],
                                         ts, True, it)
        _, w = eng.get_params()
        eng.close()
        assert np.abs(w[D_CTX:] - w0[D_CTX:]).max() > 1e-6     # the candidates' side moved
        if alpha == 0.0:
            assert np.array_equal(w[:D_CTX], w0[:D_CTX])       # bit for bit
        else:
            shrunk = w0[:D_CTX].copy()
            for i in range(1, it):
                shrunk = shrunk / (1 + _psgd_eta("optimal", HYPER["eta0"], alpha, HYPER["beta"],
                                                 HYPER["power_t"], i)[1] * alpha)
            np.testing.assert_allclose(w[:D_CTX], shrunk, rtol=1e-13, atol=0)


# ------------------------------------------------------------------ 4. evaluation entry
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4], CASES[5], CASES[6]], ids=case_id)
def test_pairs_eval_reads_and_changes_nothing(case):
    from sparsepoly_amd.pairwise import _loss_pos, restate_margins

    (X, Z, t, lams), ref = restate_case(case, 1)
    _, ts = _stacked(X, Z, t)
    eng = _engine(case, X, Z)
    try:
        for stage in range(2):
            if stage == 1:
                _epoch(eng, case, ts, 1)
            P, w = (pair_params(case)[:2], ref[0][:2])[stage]
            m = restate_margins(P, w, lams, X, Z, t, case["degree"])
            before = eng.get_params()
            sl, n_ord = eng.psgd_pairs_eval(case["degree"], case["fit_linear"], ts)
            after = eng.get_params()
            np.testing.assert_allclose(sl, _loss_pos(case["loss"], m)[0].sum(), rtol=1e-10)
            assert n_ord == int((m > 0).sum())
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. end to end
E2E_EPOCHS = 5
E2E_KW = dict(degree=2, n_components=6, fit_lower=None, fit_linear=True, regularizer="l1",
              alpha=1e-3, beta=1e-2, gamma=1e-4, eta0=0.5, learning_rate="invscaling", power_t=0.3,
              batch_size=64, max_iter=E2E_EPOCHS, tol=-1.0, n_iter_no_change=1000, shuffle=True,
              random_state=3, precision="f64")


def planted_problem():
    """(X, Z, train, held): 200 contexts (a user id and two of eight attributes), 60 candidates
    (an item id); per context the four best candidates of a planted two-tower model are the
    training interactions, the next two are held out"""
    rng = np.random.RandomState(7)
    B, Cn, r = 200, 60, 4
    order = np.argsort(-(rng.randn(B, r) @ rng.randn(Cn, r).T), axis=1)
    train = sp.csr_matrix((np.ones(B * 4), (np.repeat(np.arange(B), 4), order[:, :4].ravel())),
                          shape=(B, Cn))
    held = sp.csr_matrix((np.ones(B * 2), (np.repeat(np.arange(B), 2), order[:, 4:6].ravel())),
                         shape=(B, Cn))
    d = B + 8 + Cn
    attr = np.stack([rng.choice(8, 2, replace=False) for _ in range(B)])
    X = sp.csr_matrix((np.ones(3 * B),
                       (np.repeat(np.arange(B), 3),
                        np.column_stack([np.arange(B), B + attr]).ravel())), shape=(B, d))
    Z = sp.csr_matrix((np.ones(Cn), (np.arange(Cn), B + 8 + np.arange(Cn))), shape=(Cn, d))
    return X, Z, train, held


def planted_restated():
    """the restated fit of E2E_KW on the planted problem: the same draws in the same order as
    ``SparseFactorizationMachineRanker.fit``.  -> (P_init, P, w, lams, it, mean losses)"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd.pairwise import epoch_triples, restate_pairwise_epoch

    X, Z, train, _ = planted_problem()
    d = X.shape[1]
    r2 = check_random_state(E2E_KW["random_state"])
    P = 0.01 * r2.randn(1, 6, d)
    w, lams = np.zeros(d), np.ones(6)
    P_init = P.copy()
    it, losses = 1, []
    for t in epoch_triples(r2, E2E_EPOCHS, interactions=train, n_negatives=2, resample=True,
                           shuffle=True):
        P, w, sl, it = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, "logistic", "l1", 1e-3, 1e-2,
                                              1e-4, 0.5, "invscaling", 0.3, 64, True, it)
        losses.append(float(sl) / t.shape[0])
    return P_init, P, w, lams, it, losses


def held_out_triples():
    from sklearn.utils import check_random_state

    from sparsepoly_amd.pairwise import sample_triples

    _, _, train, held = planted_problem()
    return sample_triples(held, 3, check_random_state(12), exclude=train)


def test_ranker_fit_end_to_end():
    """Resampled negatives and shuffled triples under one random_state on both sides; every
    comparison is against the restatement computed here."""
    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import _loss_pos, restate_margins

    X, Z, train, held = planted_problem()
    d = X.shape[1]
    est = SparseFactorizationMachineRanker(**E2E_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=train, n_negatives=2, resample=True)
    P_init, P, w, lams, it, losses = planted_restated()
    assert est.it_ == it == 1 + E2E_EPOCHS * 25 and est.n_iter_ == E2E_EPOCHS - 1
    print("max|dP| = %.3e, max|dw| = %.3e, losses %s"
          % (np.abs(est.P_ - P).max(), np.abs(est.w_ - w).max(), losses))
    np.testing.assert_allclose(est.P_, P, rtol=0, atol=1e-9 * E2E_EPOCHS)
    np.testing.assert_allclose(est.w_, w, rtol=0, atol=1e-9 * E2E_EPOCHS)
    # held-out triples: the loss at initialisation, the restated parameters' and the device's
    th = held_out_triples()
    loss0 = _loss_pos("logistic", restate_margins(P_init, np.zeros(d), lams, X, Z, th, 2))[0].mean()
    assert losses[-1] < losses[0] < loss0
    m = restate_margins(P, w, lams, X, Z, th, 2)
    assert np.abs(m).min() > 1e-6    # (no held-out margin near zero: the share compares exactly)
    mean_loss, share = est.pairwise_loss(X, Z, th)
    # margins move by at most ~ (parameter bar) x (entries of a summed row x components)
    np.testing.assert_allclose(mean_loss, _loss_pos("logistic", m)[0].mean(), rtol=1e-7)
    assert share == (m > 0).mean()
    # full-catalogue metrics: the values the restated parameters give through the same call
    got = est.rank_metrics(X, Z, held, exclude=train, ks=(5, 10))
    twin = SparseFactorizationMachineRanker(**E2E_KW)
    twin.P_, twin.w_, twin.lams_ = np.ascontiguousarray(P, dtype=np.double), w.copy(), lams
    want = twin.rank_metrics(X, Z, held, exclude=train, ks=(5, 10))
    for name in ("recall@5", "recall@10", "ndcg@10", "mrr", "auc"):
        np.testing.assert_allclose(got[name], want[name], rtol=0, atol=1e-12, err_msg=name)
    rows = X[:5] + Z[:5]
    np.testing.assert_allclose(est.decision_function(rows), twin.decision_function(rows), rtol=0,
                               atol=1e-7)
    # a second fit with warm_start continues it_
    est.set_params(warm_start=True, max_iter=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=train, n_negatives=2)
    assert est.it_ == it + 25


# ------------------------------------------------------------------ 6. error codes
def test_error_codes_behind_the_c_abi():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    case = CASES[0]
    X, Z, t = pair_problem()
    S, ts = _stacked(X, Z, t)
    eng = _engine(case, X, Z)

    def epoch(tr, batch=8, it=1, lr=1):
        tr = np.ascontiguousarray(tr, dtype=np.int32)
        itc, sl = C.c_int64(it), C.c_double()
        return eng._lib.spfm_psgd_pairs_epoch(eng._h, 2, 0.01, 0.5, 0.003, 0.05, lr, 0.8, batch,
                                              tr.ctypes.data_as(_capi._ip), tr.shape[0], 1,
                                              C.byref(itc), C.byref(sl))

    def evaluate(tr):
        tr = np.ascontiguousarray(tr, dtype=np.int32)
        sl, no = C.c_double(), C.c_int64()
        return eng._lib.spfm_psgd_pairs_eval(eng._h, 2, 1, tr.ctypes.data_as(_capi._ip),
                                             tr.shape[0], C.byref(sl), C.byref(no))

    before = eng.get_params()
    overlap = ts.copy()
    overlap[5] = (4, 4, N_CTX + 1)         # a context row in a candidate's place
    same = ts.copy()
    same[9, 2] = same[9, 1]
    for bad in (overlap, same):
        assert epoch(bad) == _capi.SPFM_ERR_INVALID
        assert evaluate(bad) == _capi.SPFM_ERR_INVALID
    for val in (-1, S.shape[0]):
        out = ts.copy()
        out[11, 0] = val
        assert epoch(out) == _capi.SPFM_ERR_INVALID
        assert evaluate(out) == _capi.SPFM_ERR_INVALID
    assert epoch(ts, batch=0) == _capi.SPFM_ERR_INVALID
    assert epoch(ts, it=0) == _capi.SPFM_ERR_INVALID
    assert epoch(ts, lr=4) == _capi.SPFM_ERR_INVALID
    with pytest.raises(ValueError, match="column"):
        eng.psgd_pairs_epoch(2, 0.01, 0.5, 0.003, 0.05, "optimal", 0.8, 8, overlap, True, 1)
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert epoch(ts) == _capi.SPFM_OK      # the same handle still trains
    eng.close()
    # a handle configured for another solver
    P0, w0, lams = pair_params(case)
    eng = HipEngine(0, "f64")
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0, w0, lams)
    eng.configure("pcd", "logistic", "l1", 2)
    before = eng.get_params()
    assert epoch(ts) == _capi.SPFM_ERR_INVALID
    assert evaluate(ts) == _capi.SPFM_ERR_INVALID
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    eng.close()
