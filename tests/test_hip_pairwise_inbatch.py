"""In-batch softmax of the ranking fit on the device against the NumPy
restatement; problem and cases from ``tests/test_pairwise_inbatch_host.py``.  Tolerances are the
psgd bars of ``tests/test_hip_pairwise.py``: P and w to 1e-9 (f64 handle) / 5e-5 (f32), sum_loss
to 1e-10 / 1e-5 relative, ``it`` exactly."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
from test_pairwise_host import GAMMA, HYPER, N_CAND, N_CTX
from test_pairwise_inbatch_host import CASES, case_id, restate_case

pytestmark = pytest.mark.gpu

P_ATOL = {"f64": 1e-9, "f32": 5e-5}
SL_RTOL = {"f64": 1e-10, "f32": 1e-5}


def _stacked(X, Z, pairs):
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    return S, (pairs + np.array([0, X.shape[0]])).astype(np.int32)


def _engine(case, opts=(), comm=False):
    from sparsepoly_amd.engine import HipEngine

    (X, Z, pairs, P0, w0, lams), _ = restate_case(case)
    S, ps = _stacked(X, Z, pairs)
    eng = HipEngine(0, case["precision"])
    for key, val in opts:
        eng.set_option(key, val)
    if comm:
        eng.comm_init(HipEngine.comm_unique_id(), 1, 0)
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0.copy(), w0.copy(), lams)
    eng.configure("psgd", "logistic", case["reg"], case["degree"])
    return eng, ps


def _step(case, batch=None):
    return (case["degree"], HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]], HYPER["eta0"],
            HYPER["learning_rate"], HYPER["power_t"], case["batch"] if batch is None else batch)


def _close(case, P, w, Pr, wr):
    np.testing.assert_allclose(P, Pr, rtol=0, atol=P_ATOL[case["precision"]])
    np.testing.assert_allclose(w, wr, rtol=0, atol=P_ATOL[case["precision"]])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_two_epochs_against_the_restatement(case):
    (X, Z, pairs, P0, w0, lams), ref = restate_case(case)
    eng, ps = _engine(case)
    it = 1
    try:
        for ep in range(2):
            sl, it = eng.psgd_inbatch_epoch(*_step(case), ps, case["fit_linear"], it)
            P, w = eng.get_params()
            Pr, wr, slr, itr = ref[ep]
            print("epoch %d: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
                  % (ep + 1, np.abs(P - Pr).max(), np.abs(w - wr).max(),
                     abs(sl - slr) / max(abs(slr), 1e-300)))
            assert it == itr
            np.testing.assert_allclose(sl, slr, rtol=SL_RTOL[case["precision"]])
            _close(case, P, w, Pr, wr)
        assert np.abs(P - P0).max() > 1e-4     # it did train (batch 1: by the shrink alone)
    finally:
        eng.close()


def test_graph_replay_agrees_with_eager_launches():
    """batch 4: 38 minibatches per epoch, one replayed run of 32 and 6 single table-driven
    launches; both routes against the restatement (the atomics are not ordered)"""
    case = CASES[0]
    _, ref = restate_case(case, 4)
    for opts in ((), (("psgd_eager", 1),)):
        eng, ps = _engine(case, opts)
        try:
            it = 1
            for ep in range(2):
                sl, it = eng.psgd_inbatch_epoch(*_step(case, 4), ps, case["fit_linear"], it)
                np.testing.assert_allclose(sl, ref[ep][2], rtol=SL_RTOL["f64"])
            assert it == ref[1][3] == 1 + 2 * 38
            assert eng.get_option("psgd_eager") == (1 if opts else 0)
            _close(case, *eng.get_params(), ref[1][0], ref[1][1])
        finally:
            eng.close()


def test_eval_gives_the_loss_and_leaves_the_parameters_bit_for_bit():
    from sparsepoly_amd.pairwise import restate_inbatch_gradient

    case = CASES[5]
    (X, Z, pairs, P0, w0, lams), _ = restate_case(case)
    want = sum(restate_inbatch_gradient(P0, w0, lams, X, Z, pairs[a:a + case["batch"]],
                                        case["degree"])[0].sum()
               for a in range(0, len(pairs), case["batch"]))
    eng, ps = _engine(case)
    try:
        before = eng.get_params()
        sl = eng.psgd_inbatch_eval(case["degree"], case["batch"], ps)
        after = eng.get_params()
        np.testing.assert_allclose(sl, want, rtol=SL_RTOL["f64"])
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
    finally:
        eng.close()


def _codes(eng, ps, batch=8):
    """the status of both entries on the raw library"""
    pp = ps.ctypes.data_as(C.POINTER(C.c_int32))
    itc, sl = C.c_int64(1), C.c_double()
    ep = eng._lib.spfm_psgd_inbatch_epoch(eng._h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, batch, pp,
                                          ps.shape[0], 1, C.byref(itc), C.byref(sl))
    ev = eng._lib.spfm_psgd_inbatch_eval(eng._h, 2, batch, pp, ps.shape[0], C.byref(sl))
    assert itc.value == 1
    return ep, ev


def test_every_error_code_and_untouched_parameters():
    from sparsepoly_amd import _capi

    case = CASES[0]
    inv, uns = (_capi.SPFM_ERR_INVALID,) * 2, (_capi.SPFM_ERR_UNSUPPORTED,) * 2
    eng, ps = _engine(case)
    try:
        before = eng.get_params()
        outside = ps.copy()
        outside[3, 1] = N_CTX + N_CAND
        swapped = np.concatenate([ps, ps[:1, ::-1]])  # a candidate row as a context: shared columns
        assert _codes(eng, outside) == inv
        assert _codes(eng, swapped) == inv
        assert _codes(eng, ps[:0]) == inv
        assert _codes(eng, ps, batch=0) == inv
        eng.psgd_pairs_set_deterministic(1)
        assert _codes(eng, ps) == uns
        eng.psgd_pairs_set_deterministic(0)
        eng.set_sample_weight(np.ones(N_CTX + N_CAND))
        assert _codes(eng, ps) == uns
        assert all(np.array_equal(a, b) for a, b in zip(before, eng.get_params()))
    finally:
        eng.close()
    eng, ps = _engine(case, comm=True)
    try:
        assert _codes(eng, ps) == uns
    finally:
        eng.close()


def test_estimator_fit_and_in_batch_loss_against_the_rebuilt_loop():
    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import (_prepare_pairs, epoch_pairs, restate_inbatch_epoch,
                                         restate_inbatch_gradient)
    from sklearn.utils import check_random_state

    (X, Z, pairs, _, _, _), _ = restate_case(CASES[0])
    I = sp.csr_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(N_CTX, N_CAND))
    I.sum_duplicates()
    kw = dict(degree=2, n_components=8, regularizer="l1", alpha=1e-2, beta=0.5, gamma=0.003,
              eta0=0.05, max_iter=2, tol=-1e9, shuffle=True, batch_size=64,
              learning_rate="adagrad", random_state=7, precision="f64")
    est = SparseFactorizationMachineRanker(**kw).fit(X, Z, interactions=I, sampler="in_batch",
                                                     objective="softmax")
    # the same draws from the same seed, then the restated epochs
    rng = check_random_state(7)
    Xa, Za = _prepare_pairs(est, X, Z)
    P = 0.01 * rng.randn(1, 8, Xa.shape[1])
    w, lams = np.zeros(Xa.shape[1]), np.ones(8)
    pos = np.stack([np.repeat(np.arange(N_CTX), np.diff(I.indptr)), I.indices], axis=1)
    it, acc = 1, None
    for pr in epoch_pairs(rng, 2, pos, True):
        P, w, _, it, acc = restate_inbatch_epoch(
            P, w, lams, Xa, Za, pr, 2, "l1", 1e-2, 0.5, 0.003, 0.05, est._base_rate(), 1.0, 64,
            True, it, adaptive=True, acc=acc)
    assert est.it_ == it
    np.testing.assert_allclose(est.P_, P, rtol=0, atol=1e-9)
    np.testing.assert_allclose(est.w_, w, rtol=0, atol=1e-9)
    want = sum(restate_inbatch_gradient(P, w, lams, Xa, Za, pos[a:a + 50], 2)[0].sum()
               for a in range(0, len(pos), 50)) / len(pos)
    np.testing.assert_allclose(est.in_batch_loss(X, Z, pos, 50), want, rtol=1e-10)
