"""Listwise ranking fit on the device against the NumPy restatement of
``sparsepoly_amd/pairwise.py`` and against the tested pairwise path.  Needs a real MI355X:
``pytest -m gpu``.  The problem and the cases come from ``tests/test_pairwise_list_host.py``,
which also shows that no list used here is a near-tie (the empty context's list apart).

Tolerances are the psgd bars of ``tests/test_hip_pairwise.py``: P and w to 1e-9 (f64 handle) /
5e-5 (f32), sum_loss to 1e-10 / 1e-5 relative, ``it`` exactly."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from test_pairwise_host import GAMMA, HYPER, N_CAND, N_CTX
from test_pairwise_list_host import CASES, case_id, list_problem, restate_case

pytestmark = pytest.mark.gpu

P_ATOL = {"f64": 1e-9, "f32": 5e-5}
SL_RTOL = {"f64": 1e-10, "f32": 1e-5}


def _stacked(X, Z, t):
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    return S, (t + np.array([0, X.shape[0], X.shape[0]])).astype(np.int32)


def _engine(case, opts=()):
    from sparsepoly_amd.engine import HipEngine

    (X, Z, t, P0, w0, lams), _ = restate_case(case)
    S, _ = _stacked(X, Z, t)
    eng = HipEngine(0, case["precision"])
    for key, val in opts:
        eng.set_option(key, val)
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0.copy(), w0.copy(), lams)
    eng.configure("psgd", case["loss"], case["reg"], case["degree"])
    return eng


def _step(case, batch=None):
    return (case["degree"], HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]], HYPER["eta0"],
            HYPER["learning_rate"], HYPER["power_t"], case["batch"] if batch is None else batch)


def _epoch(eng, case, ts, it):
    return eng.psgd_lists_epoch(*_step(case), ts, case["M"], case["objective"],
                                case["fit_linear"], it)


def _close(case, P, w, Pr, wr, scale=1):
    np.testing.assert_allclose(P, Pr, rtol=0, atol=scale * P_ATOL[case["precision"]])
    np.testing.assert_allclose(w, wr, rtol=0, atol=scale * P_ATOL[case["precision"]])


# ------------------------------------------------------------------ 1. epochs vs the restatement
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_and_two_epochs_against_the_restatement(case):
    (X, Z, t, P0, w0, lams), ref = restate_case(case)
    _, ts = _stacked(X, Z, t)
    eng = _engine(case)
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
            _close(case, P, w, Pr, wr)
        assert np.abs(P - P0).max() > 1e-4     # it did train
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. 'list' vs the pairwise path
@pytest.mark.parametrize("case", [c for c in CASES if c["objective"] == "list"], ids=case_id)
def test_list_epoch_is_the_pairwise_epoch_with_batch_times_M(case):
    (X, Z, t, P0, w0, lams), _ = restate_case(case)
    _, ts = _stacked(X, Z, t)
    M, prec = case["M"], case["precision"]
    a, b = _engine(case), _engine(case)
    try:
        ita = itb = 1
        for ep in range(2):
            sla, ita = _epoch(a, case, ts, ita)
            slb, itb = b.psgd_pairs_epoch(*_step(case, case["batch"] * M), ts,
                                          case["fit_linear"], itb)
            (Pa, wa), (Pb, wb) = a.get_params(), b.get_params()
            print("epoch %d: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
                  % (ep + 1, np.abs(Pa - Pb).max(), np.abs(wa - wb).max(),
                     abs(sla * M - slb) / abs(slb)))
            assert ita == itb
            np.testing.assert_allclose(sla * M, slb, rtol=SL_RTOL[prec])
            _close(case, Pa, wa, Pb, wb)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 3. graph replay vs eager
@pytest.mark.parametrize("ci", [0, 2], ids=["l1-softmax", "squaredl12-list"])
def test_graph_replay_agrees_with_eager_launches(ci):
    """batch 1: 60 minibatches per epoch, one replayed run of 32 and 28 single launches.  The
    squared-norm prox replays from its second (warm) epoch on."""
    case = CASES[ci]
    (X, Z, t, P0, w0, lams), _ = restate_case(case)
    _, ts = _stacked(X, Z, t)
    res = {}
    for mode, opts in (("graph", ()), ("eager", (("psgd_eager", 1),))):
        eng = _engine(case, opts)
        it, sls = 1, []
        for _ in range(3):
            sl, it = eng.psgd_lists_epoch(*_step(case, 1), ts, case["M"], case["objective"],
                                          case["fit_linear"], it)
            sls.append(sl)
        res[mode] = (eng.get_params(), np.array(sls), it, eng.get_option("psgd_redone"))
        eng.close()
    print("psgd_redone: graph %d, eager %d" % (res["graph"][3], res["eager"][3]))
    assert res["eager"][3] == 0
    assert res["graph"][2] == res["eager"][2] == 1 + 3 * 60
    np.testing.assert_allclose(res["graph"][1], res["eager"][1], rtol=1e-10)
    _close(case, *res["graph"][0], *res["eager"][0])
    assert np.abs(res["graph"][0][0] - P0).max() > 1e-4


# ------------------------------------------------------------------ 4. the sampled route
def _interactions(t, M):
    head = np.unique(t[::M, :2], axis=0)
    return sp.csr_matrix((np.ones(len(head)), (head[:, 0], head[:, 1])), shape=(N_CTX, N_CAND))


@pytest.mark.parametrize("ci,n_candidates", [(0, 1), (4, 4)], ids=["uniform", "dynamic"])
def test_sampled_lists_equal_the_uploaded_epoch_of_the_downloaded_triples(ci, n_candidates):
    case = CASES[ci]
    (X, Z, t, P0, w0, lams), _ = restate_case(case)
    M = case["M"]
    I = _interactions(t, M)
    Q = I.nnz
    perm = np.random.RandomState(4).permutation(Q).astype(np.int32)
    for order in (None, perm):
        a, b = _engine(case), _engine(case)
        try:
            a.psgd_pairs_set_sampler(N_CTX, N_CAND, I)
            m, ts, _ = a.psgd_pairs_sample(case["degree"], M, n_candidates, 64 * n_candidates, 9,
                                           0)
            assert m == Q * M and np.array_equal(ts[::M, :2].repeat(M, axis=0), ts[:, :2])
            sla, ita = a.psgd_lists_epoch_sampled(*_step(case), M, case["objective"],
                                                  case["fit_linear"], 1, list_order=order)
            visit = ts if order is None else ts.reshape(Q, M, 3)[order].reshape(-1, 3)
            slb, itb = _epoch(b, case, visit, 1)
            assert ita == itb
            np.testing.assert_allclose(sla, slb, rtol=SL_RTOL[case["precision"]])
            _close(case, *a.get_params(), *b.get_params())
            # the resident list survives its epoch: a second one runs over the same lists
            sla, ita = a.psgd_lists_epoch_sampled(*_step(case), M, case["objective"],
                                                  case["fit_linear"], ita, list_order=order)
            slb, itb = _epoch(b, case, visit, itb)
            np.testing.assert_allclose(sla, slb, rtol=SL_RTOL[case["precision"]])
            _close(case, *a.get_params(), *b.get_params())
        finally:
            a.close()
            b.close()


def test_a_mismatched_sampling_is_refused():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import SpfmError

    case = CASES[0]
    (X, Z, t, P0, w0, lams), _ = restate_case(case)
    M = case["M"]
    I = _interactions(t, M)
    eng = _engine(case)

    def sampled(n_neg, list_order=None, list_loss=0, batch=7):
        itc, sl = C.c_int64(1), C.c_double()
        o = None if list_order is None else np.ascontiguousarray(list_order, dtype=np.int32)
        return eng._lib.spfm_psgd_lists_epoch_sampled(
            eng._h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, batch, n_neg, list_loss,
            None if o is None else o.ctypes.data_as(_capi._ip), 1, C.byref(itc), C.byref(sl))

    try:
        before = eng.get_params()
        assert sampled(M) == _capi.SPFM_ERR_INVALID                 # no sampler, no resident list
        eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I)
        assert sampled(M) == _capi.SPFM_ERR_INVALID                 # nothing sampled yet
        eng.psgd_pairs_sample(2, M, 1, 64, 9, 0, order=np.random.RandomState(0).permutation(
            I.nnz * M))
        assert sampled(M) == _capi.SPFM_ERR_INVALID                 # scattered by a slot order
        eng.psgd_pairs_sample(2, M + 1, 1, 64, 9, 0)
        assert sampled(M) == _capi.SPFM_ERR_INVALID                 # another n_negatives
        eng.psgd_pairs_sample(2, M, 1, 64, 9, 0)
        twice = np.arange(I.nnz)
        twice[1] = 0
        assert sampled(M, list_order=twice) == _capi.SPFM_ERR_INVALID
        assert sampled(M, list_order=np.arange(I.nnz) + 1) == _capi.SPFM_ERR_INVALID
        assert sampled(M, list_loss=2) == _capi.SPFM_ERR_INVALID
        assert sampled(M, batch=0) == _capi.SPFM_ERR_INVALID
        after = eng.get_params()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert sampled(M) == _capi.SPFM_OK                          # the list is still resident
        # an upload overwrites the resident list
        _, ts = _stacked(X, Z, t)
        _epoch(eng, case, ts, 1)
        assert sampled(M) == _capi.SPFM_ERR_INVALID
        with pytest.raises((SpfmError, ValueError)):
            eng.psgd_lists_epoch_sampled(*_step(case), M, "softmax", True, 1)
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. evaluation entry
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3], CASES[4], CASES[5], CASES[6],
                                  CASES[9]], ids=case_id)
def test_lists_eval_reads_and_changes_nothing(case):
    from sparsepoly_amd.pairwise import _list_coefs, restate_list_scores

    (X, Z, t, P0, w0, lams), ref = restate_case(case)
    _, ts = _stacked(X, Z, t)
    M, prec = case["M"], case["precision"]
    capped = np.diff(X.indptr)[t[::M, 0]] == 0      # the lists the host test's cap leaves out
    assert capped.sum() == 1
    eng = _engine(case)
    try:
        for stage in range(2):
            if stage == 1:
                _epoch(eng, case, ts, 1)
            P, w = ((P0, w0), ref[0][:2])[stage]
            s = restate_list_scores(P, w, lams, X, Z, t, M, case["degree"])
            val, _ = _list_coefs(s, case["objective"], case["loss"])
            first = s[:, 0] > s[:, 1:].max(axis=1)
            before = eng.get_params()
            sl, n_first = eng.psgd_lists_eval(case["degree"], case["fit_linear"], ts, M,
                                              case["objective"])
            after = eng.get_params()
            np.testing.assert_allclose(sl, val.sum(), rtol=SL_RTOL[prec])
            lo = int(first[~capped].sum())
            assert lo <= n_first <= lo + int(capped.sum())
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. error codes
def test_error_codes_behind_the_c_abi():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    case = CASES[0]
    (X, Z, t, P0, w0, lams), _ = restate_case(case)
    S, ts = _stacked(X, Z, t)
    M = case["M"]
    eng = _engine(case)

    def epoch(tr, n_neg=M, list_loss=0, batch=8, it=1, lr=1, h=None):
        tr = np.ascontiguousarray(tr, dtype=np.int32)
        itc, sl = C.c_int64(it), C.c_double()
        return eng._lib.spfm_psgd_lists_epoch(
            (h or eng)._h, 2, 0.01, 0.5, 0.003, 0.05, lr, 0.8, batch,
            tr.ctypes.data_as(_capi._ip), tr.shape[0], n_neg, list_loss, 1, C.byref(itc),
            C.byref(sl))

    def evaluate(tr, n_neg=M, list_loss=0, h=None):
        tr = np.ascontiguousarray(tr, dtype=np.int32)
        sl, nf = C.c_double(), C.c_int64()
        return eng._lib.spfm_psgd_lists_eval((h or eng)._h, 2, 1, tr.ctypes.data_as(_capi._ip),
                                             tr.shape[0], n_neg, list_loss, C.byref(sl),
                                             C.byref(nf))

    before = eng.get_params()
    overlap = ts.copy()
    overlap[3:6, 0] = 4
    overlap[3:6, 1] = 4                      # a context row in a candidate's place
    same = ts.copy()
    same[10, 2] = same[10, 1]                # plus == minus
    outside = ts.copy()
    outside[12:15, 0] = S.shape[0]
    anchor = ts.copy()
    anchor[7, 0] = (anchor[7, 0] + 1) % N_CTX   # a group whose rows differ in anchor
    plus = ts.copy()
    plus[8, 1] = N_CTX + (plus[8, 1] - N_CTX + 1) % N_CAND
    if plus[8, 1] == plus[8, 2]:
        plus[8, 1] = N_CTX + (plus[8, 1] - N_CTX + 1) % N_CAND
    for bad in (overlap, same, outside, anchor, plus, ts[:-1]):
        assert epoch(bad) == _capi.SPFM_ERR_INVALID
        assert evaluate(bad) == _capi.SPFM_ERR_INVALID
    for n_neg in (0, -1, 64):
        assert epoch(ts[:64 * 2], n_neg=n_neg) == _capi.SPFM_ERR_INVALID
        assert evaluate(ts[:64 * 2], n_neg=n_neg) == _capi.SPFM_ERR_INVALID
    for list_loss in (-1, 2):
        assert epoch(ts, list_loss=list_loss) == _capi.SPFM_ERR_INVALID
        assert evaluate(ts, list_loss=list_loss) == _capi.SPFM_ERR_INVALID
    assert epoch(ts, batch=0) == _capi.SPFM_ERR_INVALID
    assert epoch(ts, it=0) == _capi.SPFM_ERR_INVALID
    assert epoch(ts, lr=4) == _capi.SPFM_ERR_INVALID
    with pytest.raises(ValueError, match="grouped"):
        eng.psgd_lists_epoch(*_step(case), anchor, M, "softmax", True, 1)
    with pytest.raises(ValueError, match="list_loss"):
        eng.psgd_lists_epoch(*_step(case), ts, M, "warp", True, 1)
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert epoch(ts) == _capi.SPFM_OK        # the same handle still trains
    assert np.abs(eng.get_params()[0] - before[0]).max() > 1e-6
    eng.close()
    # a handle configured for another solver
    other = HipEngine(0, "f64")
    other.set_data(S, np.zeros(S.shape[0]))
    other.set_params(P0.copy(), w0.copy(), lams)
    other.configure("pcd", "logistic", "l1", 2)
    before = other.get_params()
    assert epoch(ts, h=other) == _capi.SPFM_ERR_INVALID
    assert evaluate(ts, h=other) == _capi.SPFM_ERR_INVALID
    after = other.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    other.close()


def test_a_handle_with_a_communicator_is_unsupported():
    """a 1-rank communicator makes the handle a distributed one: the three list entries answer
    SPFM_ERR_UNSUPPORTED before anything else and leave the parameters as they were"""
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    case = CASES[0]
    (X, Z, t, P0, w0, lams), _ = restate_case(case)
    S, ts = _stacked(X, Z, t)
    M = case["M"]
    eng = HipEngine(0, "f64")
    try:
        eng.comm_init(HipEngine.comm_unique_id(), 1, 0)
        eng.set_data(S, np.zeros(S.shape[0]))
        eng.set_params(P0.copy(), w0.copy(), lams)
        eng.configure("psgd", case["loss"], case["reg"], case["degree"])
        before = eng.get_params()
        tp = ts.ctypes.data_as(_capi._ip)
        for list_loss in (0, 1):
            itc, sl, nf = C.c_int64(1), C.c_double(), C.c_int64()
            assert eng._lib.spfm_psgd_lists_epoch(
                eng._h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, 8, tp, ts.shape[0], M, list_loss, 1,
                C.byref(itc), C.byref(sl)) == _capi.SPFM_ERR_UNSUPPORTED
            assert eng._lib.spfm_psgd_lists_epoch_sampled(
                eng._h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, 8, M, list_loss, None, 1,
                C.byref(itc), C.byref(sl)) == _capi.SPFM_ERR_UNSUPPORTED
            assert eng._lib.spfm_psgd_lists_eval(
                eng._h, 2, 1, tp, ts.shape[0], M, list_loss, C.byref(sl),
                C.byref(nf)) == _capi.SPFM_ERR_UNSUPPORTED
            assert itc.value == 1
        with pytest.raises(NotImplementedError, match="several ranks"):
            _epoch(eng, case, ts, 1)
        with pytest.raises(NotImplementedError, match="several ranks"):
            eng.psgd_lists_eval(2, True, ts, M, "softmax")
        after = eng.get_params()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. the estimator
FIT_EPOCHS = 3
FIT_KW = dict(degree=2, n_components=6, fit_lower=None, fit_linear=True, regularizer="l1",
              alpha=1e-3, beta=1e-2, gamma=1e-4, eta0=0.5, learning_rate="invscaling", power_t=0.3,
              batch_size=8, max_iter=FIT_EPOCHS, tol=-1.0, n_iter_no_change=1000, shuffle=True,
              random_state=3, precision="f64")


def _fit_problem():
    X, Z, t = list_problem(1, 40)
    return X, Z, _interactions(t, 1)


def test_softmax_fit_with_dynamic_negatives_matches_the_rebuilt_loop():
    """The estimator's loop rebuilt from the restatements under the same random_state: the
    parameter draw, the sampler's seed, per epoch the permutation of the lists, the dynamic
    negatives at the epoch's first parameters, the list epoch."""
    from sklearn.utils import check_random_state

    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import (_list_coefs, restate_list_epoch, restate_list_scores,
                                         restate_sample)

    X, Z, I = _fit_problem()
    M, NC = 4, 3
    est = SparseFactorizationMachineRanker(**FIT_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=I, n_negatives=M, sampler="dynamic", n_candidates=NC,
                objective="softmax")
    d, Q = X.shape[1], I.nnz
    rng = check_random_state(FIT_KW["random_state"])
    P = 0.01 * rng.randn(1, 6, d)
    w, lams = np.zeros(d), np.ones(6)
    seed = rng.randint(0, 2 ** 31 - 1)
    it = 1
    for ep in range(FIT_EPOCHS):
        order = rng.permutation(Q)
        t, _, gap = restate_sample(P, w, lams, X, Z, I, 2, M, NC, 64 * NC, seed, ep)
        assert gap.min() > 1e-7      # the device's choice among the drawn candidates is safe
        t = t.reshape(Q, M, 3)[order].reshape(-1, 3)
        P, w, sl, it = restate_list_epoch(P, w, lams, X, Z, t, M, 2, "softmax", "logistic", "l1",
                                          1e-3, 1e-2, 1e-4, 0.5, "invscaling", 0.3, 8, True, it)
    assert est.it_ == it == 1 + FIT_EPOCHS * -(-Q // 8) and est.n_iter_ == FIT_EPOCHS - 1
    print("max|dP| = %.3e, max|dw| = %.3e" % (np.abs(est.P_ - P).max(), np.abs(est.w_ - w).max()))
    np.testing.assert_allclose(est.P_, P, rtol=0, atol=1e-9 * FIT_EPOCHS)
    np.testing.assert_allclose(est.w_, w, rtol=0, atol=1e-9 * FIT_EPOCHS)
    # list_loss on the fitted object
    th = t[:20 * M]
    s = restate_list_scores(P, w, lams, X, Z, th, M, 2)
    gapf = np.abs(s[:, 0] - s[:, 1:].max(axis=1))
    assert gapf.min() > 1e-6
    mean_loss, share = est.list_loss(X, Z, th, M, "softmax")
    np.testing.assert_allclose(mean_loss, _list_coefs(s, "softmax", "logistic")[0].mean(),
                               rtol=1e-7)
    assert share == (s[:, 0] > s[:, 1:].max(axis=1)).mean()
    mean_list, _ = est.list_loss(X, Z, th, M, "list")
    np.testing.assert_allclose(mean_list, _list_coefs(s, "list", "logistic")[0].mean(), rtol=1e-7)


def test_objective_pairwise_is_the_fit_without_the_keyword():
    """bit for bit.  batch_size = 1: a minibatch is one triple in one group, and the atomics of
    one group are issued in program order, so the pairwise route has one order of summation and
    two runs of it can be compared exactly."""
    from sparsepoly_amd import SparseFactorizationMachineRanker

    X, Z, I = _fit_problem()
    fits = []
    for kw in ({}, {"objective": "pairwise"}):
        est = SparseFactorizationMachineRanker(**dict(FIT_KW, batch_size=1))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est.fit(X, Z, interactions=I, n_negatives=2, **kw)
        fits.append(est)
    assert fits[0].it_ == fits[1].it_ == 1 + FIT_EPOCHS * 2 * I.nnz
    assert np.array_equal(fits[0].P_, fits[1].P_) and np.array_equal(fits[0].w_, fits[1].w_)
    assert np.abs(fits[0].P_).max() > 0


def _rebuilt(lists_of_epochs, X, Z, P, w, lams, M, objective):
    """the list epochs of FIT_KW by the restatement over the given grouped triples per epoch"""
    from sparsepoly_amd.pairwise import restate_list_epoch

    it = 1
    for t in lists_of_epochs:
        P, w, sl, it = restate_list_epoch(P, w, lams, X, Z, t, M, 2, objective, "logistic", "l1",
                                          1e-3, 1e-2, 1e-4, 0.5, "invscaling", 0.3, 8, True, it)
    return P, w, it


def _assert_fit(est, P, w, it):
    print("max|dP| = %.3e, max|dw| = %.3e" % (np.abs(est.P_ - P).max(), np.abs(est.w_ - w).max()))
    assert est.it_ == it and est.n_iter_ == FIT_EPOCHS - 1
    np.testing.assert_allclose(est.P_, P, rtol=0, atol=1e-9 * FIT_EPOCHS)
    np.testing.assert_allclose(est.w_, w, rtol=0, atol=1e-9 * FIT_EPOCHS)
    assert np.abs(est.w_).max() > 1e-4      # it did train


@pytest.mark.parametrize("objective", ["list", "softmax"])
def test_list_fit_with_host_negatives_matches_the_rebuilt_loop(objective):
    """``sampler='host'``, interactions: per epoch ``sample_triples`` and, with ``shuffle``, a
    permutation of the lists, both from the fit's ``rng`` (``epoch_lists``)"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import epoch_lists

    X, Z, I = _fit_problem()
    M = 3
    est = SparseFactorizationMachineRanker(**FIT_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=I, n_negatives=M, objective=objective)
    rng = check_random_state(FIT_KW["random_state"])
    P0 = 0.01 * rng.randn(1, 6, X.shape[1])
    lists = epoch_lists(rng, FIT_EPOCHS, interactions=I, n_negatives=M, shuffle=True)
    P, w, it = _rebuilt(lists, X, Z, P0, np.zeros(X.shape[1]), np.ones(6), M, objective)
    assert it == 1 + FIT_EPOCHS * -(-I.nnz // 8)
    _assert_fit(est, P, w, it)


def test_list_fit_on_explicit_grouped_triples_matches_the_rebuilt_loop():
    """explicit grouped ``triples``, no shuffle: every epoch visits them as given"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd import SparseFactorizationMachineRanker

    M = 5
    X, Z, t = list_problem(M, 30)
    est = SparseFactorizationMachineRanker(**dict(FIT_KW, shuffle=False))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, triples=t, n_negatives=M, objective="softmax")
    rng = check_random_state(FIT_KW["random_state"])
    P0 = 0.01 * rng.randn(1, 6, X.shape[1])
    P, w, it = _rebuilt([t] * FIT_EPOCHS, X, Z, P0, np.zeros(X.shape[1]), np.ones(6), M,
                        "softmax")
    assert it == 1 + FIT_EPOCHS * 4
    _assert_fit(est, P, w, it)


def test_list_fit_with_uniform_device_negatives_matches_the_rebuilt_loop():
    """``sampler='uniform'``, ``objective='list'``, ``resample=False``: one seed and one list
    order from ``rng``, one draw on the device (``restate_sample`` with one candidate), every
    epoch over that one list"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import restate_sample

    X, Z, I = _fit_problem()
    M, Q = 2, I.nnz
    est = SparseFactorizationMachineRanker(**FIT_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=I, n_negatives=M, sampler="uniform", resample=False,
                objective="list")
    rng = check_random_state(FIT_KW["random_state"])
    P0 = 0.01 * rng.randn(1, 6, X.shape[1])
    w0, lams = np.zeros(X.shape[1]), np.ones(6)
    seed = rng.randint(0, 2 ** 31 - 1)
    order = rng.permutation(Q)
    t, _, _ = restate_sample(P0, w0, lams, X, Z, I, 2, M, 1, 64, seed, 0)
    t = t.reshape(Q, M, 3)[order].reshape(-1, 3)
    P, w, it = _rebuilt([t] * FIT_EPOCHS, X, Z, P0, w0, lams, M, "list")
    _assert_fit(est, P, w, it)
