"""Deterministic pairwise ranking fit: the fixed-order triple gradients
against the float64 NumPy restatement ``pairwise.restate_pairwise_epoch``, bit for bit against
themselves, the plan's figures and the refusals.  Needs a real MI355X: ``pytest -m gpu``.

Tolerances are the bars of ``tests/test_hip_pairwise.py`` (P and w to 1e-9 on an f64 handle, 5e-5
on f32; sum_loss to 1e-10 / 1e-5 relative; ``it`` exactly)."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

P_ATOL = {"f64": 1e-9, "f32": 5e-5}
SL_RTOL = {"f64": 1e-10, "f32": 1e-5}
N_CTX, N_CAND, D_CTX, D = 40, 12, 66, 81     # candidates: ids [66, 78), attributes 78 and 79
M = 301
STEP = (1e-2, 0.5, 0.05, "optimal", 0.8)            # alpha, beta, eta0, learning rate, power_t
GAMMA = {"l1": 0.003, "squaredl12": 1e-3}
# regname, k, degree, n_orders, batch, precision
CASES = [("l1", 3, 2, 1, 7, "f64"), ("squaredl12", 30, 3, 1, M, "f64"), ("l1", 70, 3, 2, 7, "f64"),
         ("squaredl12", 30, 4, 1, 1, "f64"), ("l1", 30, 2, 1, M, "f32"),
         ("l1", 70, 2, 1, 2 * M, "f64")]
case_id = lambda c: "-".join(map(str, c))


@functools.lru_cache(None)
def _problem():
    """(X, Z, triples): context 0 and candidate 0 are empty, context 1 stores all 66 context
    columns (it leaves the register-resident shape), column 78 is stored in every other candidate
    (c+ and c- always share it), column 80 nowhere.  299 triples between candidates 1..11 and one
    each with candidate 0 as c+ / c-: with one batch column 78 is one run of 2 * 299 + 2 = 600
    records, pieces of 256 + 256 + 88."""
    rng = np.random.RandomState(5)
    X = sp.random(N_CTX, D, density=0.15, random_state=rng, data_rvs=rng.randn, format="lil")
    X[:, D_CTX:] = 0
    X[0, :] = 0
    X[1, :D_CTX] = 0.5 + rng.rand(D_CTX)
    Z = sp.lil_matrix((N_CAND, D))
    for c in range(1, N_CAND):
        Z[c, D_CTX + c] = 1.0
        Z[c, 78] = 0.5 + rng.rand()
        if c % 3 == 0:
            Z[c, 79] = rng.randn()
    X, Z = sp.csr_matrix(X), sp.csr_matrix(Z)
    for A in (X, Z):
        A.data[:] = np.round(A.data * 64) / 64
        A.eliminate_zeros()
    t = np.empty((M, 3), dtype=np.int32)
    t[:, 0] = rng.randint(0, N_CTX, M)
    t[:, 1] = rng.randint(1, N_CAND, M)
    t[:, 2] = 1 + (t[:, 1] - 1 + rng.randint(1, N_CAND - 1, M)) % (N_CAND - 1)
    t[:4] = [(0, 1, 2), (1, 3, 4), (5, 0, 6), (5, 6, 0)]
    return X, Z, t


def _triples(case):
    """the problem's list; a batch of 2 M visits it twice in ONE minibatch: column 78 is then a
    run of 1200 records, five pieces for the four groups of a workgroup at L = 64 (two rounds of
    the fold)"""
    return np.tile(_problem()[2], (max(1, case[4] // M), 1))


def _start(k, n_orders):
    rng = np.random.RandomState(1)
    return 0.25 * rng.randn(n_orders, k, D), 0.1 * rng.randn(D), np.sign(rng.randn(k))


def _weights():
    wt = 0.25 + np.random.RandomState(3).rand(M)
    wt[9] = 0.0
    return wt


def _device(case, det=1, options=(), weights=None, epochs=2):
    """-> (P, w, sum_loss per epoch, it, the getter's figures after every epoch)"""
    from sparsepoly_amd.engine import HipEngine

    regname, k, degree, n_orders, batch, prec = case
    X, Z, _ = _problem()
    S = sp.vstack([X, Z], format="csr")
    ts = (_triples(case) + np.array([0, N_CTX, N_CTX])).astype(np.int32)
    eng = HipEngine(0, prec)
    for key, val in options:
        eng.set_option(key, val)
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(*_start(k, n_orders))
    eng.configure("psgd", "logistic", regname, degree)
    eng.psgd_pairs_set_deterministic(det)
    alpha, beta, eta0, lr, power_t = STEP
    step = (degree, alpha, beta, GAMMA[regname], eta0, lr, power_t, batch)
    it, sls, figs = 1, [], []
    for _ in range(epochs):
        if weights is None:
            sl, it = eng.psgd_pairs_epoch(*step, ts, True, it)
        else:
            sl, it = eng.psgd_pairs_epoch_weighted(*step, ts, weights, True, it)
        sls.append(sl)
        figs.append(eng.psgd_pairs_get_deterministic())
    P, w = eng.get_params()
    eng.close()
    return P, w, np.array(sls), it, figs


@functools.lru_cache(None)
def _restated(case, weighted=False, epochs=2):
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    regname, k, degree, n_orders, batch, _ = case
    X, Z, _ = _problem()
    t = _triples(case)
    P, w, lams = _start(k, n_orders)
    alpha, beta, eta0, lr, power_t = STEP
    it, sls = 1, []
    for _ in range(epochs):
        P, w, sl, it = restate_pairwise_epoch(
            P, w, lams, X, Z, t, degree, "logistic", regname, alpha, beta, GAMMA[regname], eta0,
            lr, power_t, batch, True, it, weights=_weights() if weighted else None)
        sls.append(float(sl))
    return P, w, np.array(sls), it


def _close(case, got, want):
    prec = case[5]
    print("max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
          % (np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max(),
             np.abs(got[2] / want[2] - 1).max()))
    assert got[3] == want[3]
    np.testing.assert_allclose(got[2], want[2], rtol=SL_RTOL[prec])
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=P_ATOL[prec])
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=P_ATOL[prec])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_two_epochs_against_the_restatement(case):
    _close(case, _device(case), _restated(case))


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[5]],
                         ids=["one-batch-mich", "k70-batch7", "two-round-fold"])
def test_same_bits_on_every_run_and_route(case):
    """two fresh handles (graph replay where the driver replays: 43 minibatches are a replayed
    run of 32 and 11 single launches) and one with eager launches"""
    runs = [_device(case), _device(case), _device(case, options=(("psgd_eager", 1),))]
    for other in runs[1:]:
        for a, b in zip(runs[0][:3], other[:3]):
            assert np.array_equal(a, b)


def test_weighted_epochs_with_a_zero_weight():
    case = CASES[2]
    runs = [_device(case, weights=_weights()) for _ in range(2)]
    _close(case, runs[0], _restated(case, True))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(a, b)


def test_plan_figures():
    X, Z, t = _problem()
    ent = sp.vstack([X[t[:, 0]], Z[t[:, 1]], Z[t[:, 2]]]).tocoo()   # row % M: the position
    figs = _device(CASES[0])[4]
    runs = np.unique((ent.row % M // 7) * D + ent.col, return_counts=True)[1]
    assert figs[0] == figs[1]                    # the same list: the plan stands
    mode, segments, longest, plan_bytes = figs[0]
    assert (mode, segments, longest) == (1, runs.size, runs.max()) and plan_bytes > 0
    one = _device(CASES[1], epochs=1)[4][0]      # one batch: column 78 is one run of 600
    assert one[1:3] == (np.unique(ent.col).size, 600)
    assert _device(CASES[5], epochs=1)[4][0][2] == 1200
    assert _device(CASES[0], det=0, epochs=1)[4][0] == (0, 0, 0, 0)


def test_refusals():
    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.engine import HipEngine

    X, Z, t = _problem()
    eng = HipEngine(0, "f64")
    eng.set_data(sp.vstack([X, Z], format="csr"), np.zeros(N_CTX + N_CAND))
    eng.set_params(*_start(3, 1))
    eng.configure("psgd", "logistic", "l1", 2)
    eng.psgd_pairs_set_deterministic(1)
    with pytest.raises(NotImplementedError, match="deterministic"):   # SPFM_ERR_UNSUPPORTED
        eng.psgd_lists_epoch(2, 1e-2, 0.5, 1e-3, 0.05, "optimal", 0.8, 4,
                             np.array([[2, N_CTX + 1, N_CTX + 2]], dtype=np.int32), 1, "softmax",
                             True, 1)
    with pytest.raises(ValueError):
        eng.psgd_pairs_set_deterministic(2)
    eng.close()
    est = SparseFactorizationMachineRanker(regularizer="l1", max_iter=1)
    est.deterministic = True
    with pytest.raises(ValueError, match="lists"):
        est.fit(X, Z, triples=t[:4], objective="softmax")


def test_two_dynamic_ranker_fits_give_the_same_bits(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.engine import HipEngine

    X, Z, t = _problem()
    I = sp.csr_matrix((np.ones(M), (t[:, 0], t[:, 1])), shape=(N_CTX, N_CAND))
    drawn, sample = [], HipEngine.psgd_pairs_sample

    def recording(self, *args, **kw):
        out = sample(self, *args, **dict(kw, want_triples=True))
        drawn[-1].append(out[1])
        return out

    monkeypatch.setattr(HipEngine, "psgd_pairs_sample", recording)
    fits = []
    for _ in range(2):
        drawn.append([])
        est = SparseFactorizationMachineRanker(
            degree=2, n_components=8, regularizer="l1", alpha=1e-2, beta=0.1, gamma=1e-3,
            max_iter=2, tol=-1, n_iter_no_change=100, batch_size=16, eta0=0.05, shuffle=True,
            random_state=0, precision="f64", device=0)
        est.deterministic = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fits.append(est.fit(X, Z, interactions=I, n_negatives=2, sampler="dynamic",
                                n_candidates=4))
    assert len(drawn[0]) == 2 and all(np.array_equal(a, b) for a, b in zip(*drawn))
    assert np.array_equal(fits[0].P_, fits[1].P_) and np.array_equal(fits[0].w_, fits[1].w_)
