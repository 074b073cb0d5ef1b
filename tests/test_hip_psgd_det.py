"""Deterministic psgd: the fixed-order minibatch gradient against the
oracle, bit for bit against itself, its plan and its refusals.  Needs a real MI355X:
``pytest -m gpu``.

Tolerances are those of ``test_hip_psgd.py::test_midsize_against_oracle`` (loss sums rtol 1e-11,
P and w atol 1e-10 in f64) and, for f32 storage, of ``test_classifier_losses_midsize`` (1e-5 /
2e-5): the oracle adds a column's terms in the same order, the dot products are still trees."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N, D = 601, 40
STEP = (1e-2, 0.5, 0.05, "optimal", 0.8)            # alpha, beta, eta0, learning rate, power_t
GAMMA = {"l1": 0.003, "squaredl12": 1e-3}
# regname, k, degree, n_orders, batch, precision
CASES = [("l1", 3, 2, 1, 7, "f64"), ("squaredl12", 30, 3, 1, N, "f64"), ("l1", 70, 3, 2, 7, "f64"),
         ("squaredl12", 30, 4, 1, 1, "f64"), ("l1", 30, 2, 1, N, "f32")]


def _problem():
    """column 0 in every row but the empty one (600 entries: with batch_size = N a segment of
    256 + 256 + 88), column D - 1 nowhere, row 7 empty"""
    rng = np.random.RandomState(5)
    X = sp.random(N, D, density=0.15, random_state=rng, data_rvs=rng.randn, format="lil")
    X[:, 0] = 1.0 + rng.rand(N, 1)
    X[:, D - 1] = 0
    X[7, :] = 0
    X = sp.csr_matrix(X)
    X.data[:] = np.round(X.data * 64) / 64
    X.eliminate_zeros()
    y = rng.randn(N).astype(np.float32).astype(np.float64)
    return X, y


def _start(k, n_orders, scale=0.05):
    rng = np.random.RandomState(1)
    return scale * rng.randn(n_orders, k, D), 0.01 * rng.randn(D), np.sign(rng.randn(k))


def _orders(epochs=3):
    rng = np.random.RandomState(2)
    return [rng.permutation(N).astype(np.int32) for _ in range(epochs)]


def _device(case, det=1, options=(), weights=None, adagrad=None, orders=None):
    from sparsepoly_amd.engine import HipEngine

    regname, k, degree, n_orders, batch, prec = case
    X, y = _problem()
    P0, w0, lams = _start(k, n_orders, 0.3 if adagrad else 0.05)
    eng = HipEngine(0, prec)
    for key, val in options:
        eng.set_option(key, val)
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "squared", regname, degree)
    if weights is not None:
        eng.set_sample_weight(weights)
    if adagrad:
        eng.psgd_set_adaptive(1, adagrad)
    eng.psgd_set_deterministic(det)
    alpha, beta, eta0, lr, power_t = STEP
    it, sls, figs = 1, [], []
    for idx in orders or _orders():
        sl, it = eng.psgd_epoch(degree, alpha, beta, GAMMA[regname], eta0,
                                "constant" if adagrad else lr, power_t, batch, idx, True, it)
        sls.append(sl)
        figs.append(eng.psgd_get_deterministic())
    P, w = eng.get_params()
    eng.close()
    return P, w, np.array(sls), it, figs


def _oracle_run(oracle, case, X, y, orders):
    regname, k, degree, n_orders, batch, _ = case
    P0, w0, lams = _start(k, n_orders)
    Po, wo = np.ascontiguousarray(P0.swapaxes(1, 2)), w0.copy()
    alpha, beta, eta0, lr, power_t = STEP
    it, sls = 1, []
    for idx in orders:
        sl, it = oracle.psgd_epoch(Po, wo, oracle.CSR(X), y, lams, degree, alpha, beta,
                                   GAMMA[regname], regname, "squared", idx, True, eta0, lr, power_t,
                                   batch, it)
        sls.append(sl)
    return Po.swapaxes(1, 2), wo, np.array(sls), it


def _close(case, got, want):
    f64 = case[5] == "f64"
    assert got[3] == want[3]
    np.testing.assert_allclose(got[2], want[2], rtol=1e-11 if f64 else 1e-5)
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-10 if f64 else 2e-5)
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-10 if f64 else 2e-5)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_against_the_oracle(oracle, case):
    X, y = _problem()
    got, want = _device(case), _oracle_run(oracle, case, X, y, _orders())
    _close(case, got, want)
    if case[5] == "f64":
        assert np.array_equal(got[0] == 0, want[0] == 0)


def test_weighted_against_the_oracle_on_replicated_rows(oracle):
    case = ("l1", 30, 2, 1, N, "f64")          # one minibatch: its weight sum is its row count
    X, y = _problem()
    orders = _orders(2)
    idx = orders[0]
    w = np.zeros(N)
    w[idx] = np.r_[np.tile([2.0, 0.0, 1.0, 1.0], N // 4), 1.0]
    rows = [np.repeat(o, w[o].astype(int)) for o in orders]   # replicated, in visiting order
    assert all(r.size == N for r in rows)
    P0, w0, lams = _start(30, 1)
    Po, wo = np.ascontiguousarray(P0.swapaxes(1, 2)), w0.copy()
    alpha, beta, eta0, lr, power_t = STEP
    it, sls = 1, []
    for r in rows:
        sl, it = oracle.psgd_epoch(Po, wo, oracle.CSR(X[r]), y[r], lams, 2, alpha, beta,
                                   GAMMA["l1"], "l1", "squared", np.arange(N, dtype=np.int32),
                                   True, eta0, lr, power_t, N, it)
        sls.append(sl)
    _close(case, _device(case, weights=w, orders=orders), (Po.swapaxes(1, 2), wo, np.array(sls), it))


def test_adagrad_against_the_restated_step(oracle):
    """the step of ``test_hip_weights.py::test_psgd_adagrad_against_the_restated_step``: the mean
    gradient of a minibatch from the oracle (no penalties, unit step), then ``_adaptive_step``"""
    from sparsepoly_amd.pairwise import _adaptive_step

    case, G0 = ("l1", 3, 2, 1, 7, "f64"), 1.0
    X, y = _problem()
    alpha, beta, eta0 = STEP[:3]
    orders = _orders(2)
    P, wl, lams = _start(3, 1, 0.3)
    acc, sls = (np.zeros((1, D)), np.zeros(D)), []
    for idx in orders:
        sls.append(0.0)
        for pos in range(0, N, 7):
            rb = idx[pos:pos + 7]
            Pc, wc = np.ascontiguousarray(P.swapaxes(1, 2)), wl.copy()
            sl, _ = oracle.psgd_epoch(Pc, wc, oracle.CSR(X[rb]), y[rb], lams, 2, 0.0, 0.0, 0.0,
                                      "l1", "squared", np.arange(rb.size, dtype=np.int32), True,
                                      1.0, "constant", 1.0, rb.size, 1)
            sls[-1] += sl
            P, wl = _adaptive_step(P, wl, P - Pc.swapaxes(1, 2), wl - wc, 1, eta0, eta0, alpha,
                                   beta, GAMMA["l1"], "l1", True, G0, acc)
    it = 1 + 2 * -(-N // 7)
    _close(case, _device(case, adagrad=G0, orders=orders), (P, wl, np.array(sls), it))


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["one-batch-mich", "k70-batch7"])
def test_same_bits_on_every_run_and_route(case):
    """two fresh handles (graph replay where the driver replays) and one with eager launches"""
    runs = [_device(case), _device(case), _device(case, options=(("psgd_eager", 1),))]
    for other in runs[1:]:
        for a, b in zip(runs[0][:3], other[:3]):
            assert np.array_equal(a, b)


def test_plan_figures():
    X, _ = _problem()
    case, idx = CASES[0], _orders(1)[0]
    figs = _device(case, orders=[idx, idx])[4]
    coo = X[idx].tocoo()                         # row = position in the visiting order
    runs = np.unique((coo.row // 7) * D + coo.col, return_counts=True)[1]
    assert figs[0] == figs[1]                    # the same order: the plan stands
    mode, segments, longest, plan_bytes = figs[0]
    assert (mode, segments, longest) == (1, runs.size, runs.max()) and plan_bytes > 0
    one = _device(CASES[1], orders=[idx])[4][0]  # batch_size = N: column 0 is one run of 600
    assert one[1:3] == (np.unique(coo.col).size, 600)
    assert _device(case, det=0, orders=[idx])[4][0] == (0, 0, 0, 0)


def test_refusals():
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.engine import HipEngine

    X, y = _problem()
    eng = HipEngine(0, "f64")
    eng.set_data(X, y)
    eng.set_params(*_start(3, 1))
    eng.configure("psgd", "logistic", "l1", 2)
    eng.psgd_set_deterministic(1)
    with pytest.raises(NotImplementedError, match="deterministic"):   # SPFM_ERR_UNSUPPORTED
        eng.psgd_pairs_epoch(2, 1e-2, 0.5, 1e-3, 0.05, "optimal", 0.8, 4,
                             np.array([[0, 1, 2]], dtype=np.int32), True, 1)
    with pytest.raises(ValueError):
        eng.psgd_set_deterministic(2)
    eng.close()
    est = SparseFactorizationMachineRegressor(solver="psgd", regularizer="l1", max_iter=1,
                                              distributed=True)
    est.deterministic = True
    with pytest.raises(ValueError, match="deterministic"):
        est.fit(X, y)


def test_two_estimator_fits_give_the_same_bits():
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    X, y = _problem()
    fits = []
    for _ in range(2):
        est = SparseFactorizationMachineRegressor(
            degree=2, n_components=8, solver="psgd", regularizer="l1", alpha=1e-2, beta=0.1,
            gamma=1e-3, max_iter=3, tol=-1, n_iter_no_change=100, batch_size=16, eta0=0.05,
            shuffle=True, random_state=0, precision="f64", device=0)
        est.deterministic = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fits.append(est.fit(X, y))
    assert np.array_equal(fits[0].P_, fits[1].P_) and np.array_equal(fits[0].w_, fits[1].w_)
