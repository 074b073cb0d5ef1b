"""Weighted fits: ``spfm_set_sample_weight`` through the C ABI, the
estimators' ``sample_weight`` / ``class_weight`` and ``fit_concurrently(sample_weights=...)``.
Needs a real MI355X: ``pytest -m gpu``.

The property pinned throughout: with integer weights the weighted fit on ``(X, y, w)`` IS the
unweighted fit on the matrix that repeats row i w_i times (``weights.replicate_rows``), up to
summation order -- so the CPU oracle, which knows no weights, fitted on the replicated rows is
the reference.  Tolerances are those of the unweighted parity tests: ``P_ATOL`` / ``TRAJ_RTOL`` of
tests/test_hip_parity.py for pcd, pbcd and cd_linear (y_pred: that file's 1e-7 / 2e-4), and the
1e-11 / 1e-10 of test_hip_psgd.py::test_midsize_against_oracle for psgd in f64.
"""
import ctypes as C
import json
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import golden_csr, load_golden

from sparsepoly_amd.weights import class_weight_vector, replicate_rows

pytestmark = pytest.mark.gpu

PREC = ["f64", "f32"]
P_ATOL = {"f64": 1e-8, "f32": 1e-4}        # tests/test_hip_parity.py
TRAJ_RTOL = {"f64": 1e-9, "f32": 1e-5}
YPRED_ATOL = {"f64": 1e-7, "f32": 2e-4}


def _g3(case):
    z = load_golden("g3_small_configs.npz")
    X = golden_csr(z)
    meta = json.loads(str(z["meta|" + case]))
    y = z["y"]
    if meta["loss"] != "squared":
        y = np.where(y > np.median(y), 1.0, -1.0)
    return X, y, meta, z["P0|" + case], z["lams|" + case]


def _integer_weights(X):
    """drawn once from {0, 1, 2, 3}; the rows of one column (the shortest non-empty one) all get
    weight 0, so that column sees no weighted row at all"""
    rng = np.random.RandomState(20)
    w = rng.randint(0, 4, size=X.shape[0]).astype(np.float64)
    Xc = sp.csc_matrix(X)
    lens = np.diff(Xc.indptr)
    j = int(np.argmin(np.where(lens > 0, lens, X.shape[0] + 1)))
    w[Xc.indices[Xc.indptr[j]:Xc.indptr[j + 1]]] = 0.0
    assert lens[j] > 0 and w.sum() > 0
    return w, j


class _Engine(object):
    """one handle driven epoch by epoch as the estimators drive it (the _Run of
    tests/test_hip_parity.py, kept open so that weights can be set and cleared between runs)"""

    def __init__(self, X, y, meta, lams, precision, schedule="colored", options=None):
        from sparsepoly_amd.engine import HipEngine

        self.meta, self.lams, self.d = meta, lams, X.shape[1]
        self.eng = HipEngine(0, precision)
        for key, val in (options or {}).items():
            self.eng.set_option(key, val)
        self.eng.set_data(X, y)
        self.schedule = schedule
        self.order = None

    def run(self, P0, n_epochs=4):
        """from the start (P0, w = 0): n_epochs of cd_linear, the lower and the top passes"""
        eng, meta = self.eng, self.meta
        k, degree = meta["k"], meta["degree"]
        eng.set_params(P0, np.zeros(self.d), self.lams)
        eng.configure(meta["solver"], meta["loss"], meta["regularizer"], degree)
        eng.init_pred(degree, False, meta.get("fit_lower", "explicit") == "explicit"
                      and degree == 3)
        if self.order is None:
            self.order = eng.set_schedule(self.schedule, np.arange(self.d, dtype=np.int32))
        self.persistent_active = eng.get_option("persistent_active")
        ic = np.arange(k, dtype=np.int32)
        self.viol, self.loss = [], []
        for it in range(n_epochs):
            v = eng.cd_linear_epoch(meta["alpha"])
            for deg in list(range(2, degree)) + [degree]:
                o = degree - deg if deg != degree else 0
                if meta["solver"] == "pcd":
                    v += eng.pcd_epoch(o, deg, meta["beta"], meta["gamma"], 1.0, ic)
                else:
                    v += eng.pbcd_epoch(o, deg, meta["beta"], meta["gamma"], 1.0)
            self.viol.append(v)
            self.loss.append(eng.loss_sum())
        self.P, self.w = eng.get_params()
        self.y_pred = eng.get_y_pred()
        return self

    def close(self):
        self.eng.close()


# ------------------------------------------------- 1. replication against the oracle (cd)
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("case", ["c2|squared", "c3|squared", "c4|squared", "c4d3|logistic",
                                  "sql21|squared_hinge", "l1|squared"])
def test_replication_against_the_oracle(oracle, case, precision):
    """cd_linear, the lower and the top passes (pcd or pbcd) with integer weights against the
    oracle on the replicated rows, fed the order the coloured engine reports."""
    X, y, meta, P0, lams = _g3(case)
    w, j0 = _integer_weights(X)
    r = _Engine(X, y, meta, lams, precision)
    r.eng.set_sample_weight(w)
    assert r.eng.sample_weight_set() and r.eng.sample_weight_sum() == w.sum()
    r.run(P0)
    r.close()
    assert r.persistent_active == 0
    assert sorted(r.order) == list(range(X.shape[1]))
    Xr, yr = replicate_rows(X, y, w)
    assert Xr.shape[0] == int(w.sum()) and Xr[:, j0].nnz == 0
    fm = oracle.OracleFM(degree=meta["degree"], loss=meta["loss"], n_components=meta["k"],
                         solver=meta["solver"], regularizer=meta["regularizer"],
                         alpha=meta["alpha"], beta=meta["beta"], gamma=meta["gamma"], tol=0,
                         fit_lower="explicit", fit_linear=True, max_iter=4,
                         feature_order=r.order)
    fm.fit(Xr, yr, P_init=P0, lams_init=lams)
    viol_o, loss_o = [h[0] for h in fm.history], [h[1] for h in fm.history]
    print("viol", r.viol, viol_o)
    print("loss", r.loss, loss_o)
    print("max |P - P_o|", np.abs(r.P - fm.P_).max(), "max |w - w_o|", np.abs(r.w - fm.w_).max())
    np.testing.assert_allclose(r.viol, viol_o, rtol=TRAJ_RTOL[precision])
    np.testing.assert_allclose(r.loss, loss_o, rtol=TRAJ_RTOL[precision])
    np.testing.assert_allclose(r.P, fm.P_, rtol=0, atol=P_ATOL[precision])
    np.testing.assert_allclose(r.w, fm.w_, rtol=0, atol=P_ATOL[precision])
    # y_pred on the rows of positive weight (a zero-weight row's is maintained too: finite)
    np.testing.assert_allclose(np.repeat(r.y_pred, w.astype(int)), fm.y_pred_, rtol=0,
                               atol=YPRED_ATOL[precision])
    assert np.all(np.isfinite(r.y_pred))


# ------------------------------------------------- 2. unit weights are today's bits
@pytest.mark.parametrize("precision", PREC)
@pytest.mark.parametrize("case", ["c2|squared", "c3|logistic", "c4|squared"])
def test_unit_weights_are_the_unweighted_bits(case, precision):
    X, y, meta, P0, lams = _g3(case)
    n = X.shape[0]
    a = _Engine(X, y, meta, lams, precision)
    a.eng.set_sample_weight(np.ones(n))
    flag, total = C.c_int(-1), C.c_double(-1.0)
    assert a.eng._lib.spfm_get_sample_weight(a.eng._h, C.byref(flag), C.byref(total)) == 0
    assert flag.value == 1 and total.value == float(n)
    a.run(P0)
    assert a.persistent_active == 0
    b = _Engine(X, y, meta, lams, precision,
                options={"persistent": 0, "pbcd_persistent": 0}).run(P0)
    b.close()
    np.testing.assert_array_equal(a.order, b.order)
    assert a.viol == b.viol and a.loss == b.loss
    np.testing.assert_array_equal(a.P, b.P)
    np.testing.assert_array_equal(a.w, b.w)
    np.testing.assert_array_equal(a.y_pred, b.y_pred)
    # cleared: a fresh set of epochs from the same start is a never-weighted handle's
    a.eng.set_sample_weight(None)
    assert a.eng._lib.spfm_get_sample_weight(a.eng._h, C.byref(flag), C.byref(total)) == 0
    assert flag.value == 0 and total.value == float(n)
    a.run(P0)
    a.close()
    assert a.persistent_active == 1
    c = _Engine(X, y, meta, lams, precision).run(P0)
    c.close()
    assert c.persistent_active == 1
    assert a.viol == c.viol and a.loss == c.loss
    np.testing.assert_array_equal(a.P, c.P)
    np.testing.assert_array_equal(a.w, c.w)
    np.testing.assert_array_equal(a.y_pred, c.y_pred)


# ------------------------------------------------- 3. psgd against the oracle
N_SG, D_SG = 256, 80


def _psgd_problem():
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(N_SG, D_SG, 6, seed=5)
    X = sp.csr_matrix(X)
    X.data[:] = np.round(X.data * 64) / 64
    lil = X.tolil()
    lil[7, :] = 0        # an empty row
    X = sp.csr_matrix(lil)
    X.eliminate_zeros()
    rng = np.random.RandomState(1)
    idx = rng.permutation(N_SG).astype(np.int32)          # ONE visiting order for both epochs
    w = np.zeros(N_SG)
    w[idx] = np.tile([2.0, 0.0, 1.0, 1.0], N_SG // 4)    # every 4 visited rows weigh 4
    rows = np.repeat(idx, w[idx].astype(int))            # the replication, in visiting order
    assert rows.size == N_SG
    return X, y, idx, w, rows, rng


def _psgd_start(rng, k, n_orders, scale=0.05):
    P0 = scale * rng.randn(n_orders, k, D_SG)
    lams = np.sign(rng.randn(k))
    w0 = 0.01 * rng.randn(D_SG)
    return P0, w0, lams


@pytest.mark.parametrize("regname,k,degree,n_orders,batch", [
    ("l1", 8, 2, 1, 32), ("squaredl12", 70, 3, 2, 64), ("l21", 16, 2, 1, 256)])
def test_psgd_against_the_oracle(oracle, regname, k, degree, n_orders, batch):
    """Two epochs; the oracle runs over the rows replicated in visiting order with the same
    batch size: a minibatch of B rows has weight sum B, so both divide by B."""
    from sparsepoly_amd.engine import HipEngine

    X, y, idx, w, rows, rng = _psgd_problem()
    P0, w0, lams = _psgd_start(rng, k, n_orders)
    gamma = {"l1": 0.003, "l21": 0.5, "squaredl12": 1e-3}[regname]
    alpha, beta, eta0, lr, power_t = 1e-2, 0.5, 0.05, "optimal", 0.8
    eng = HipEngine(0, "f64")
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "squared", regname, degree)
    eng.set_sample_weight(w)
    Po, wo = np.ascontiguousarray(P0.swapaxes(1, 2)), w0.copy()
    Xr, yr = oracle.CSR(X[rows]), y[rows]
    ar = np.arange(N_SG, dtype=np.int32)
    it_d = it_o = 1
    for ep in range(2):
        sl_d, it_d = eng.psgd_epoch(degree, alpha, beta, gamma, eta0, lr, power_t, batch, idx,
                                    True, it_d)
        sl_o, it_o = oracle.psgd_epoch(Po, wo, Xr, yr, lams, degree, alpha, beta, gamma, regname,
                                       "squared", ar, True, eta0, lr, power_t, batch, it_o)
        print("epoch", ep, "sum_loss", sl_d, sl_o)
        assert it_d == it_o
        np.testing.assert_allclose(sl_d, sl_o, rtol=1e-11)
    Pd, wd = np.empty_like(P0), np.empty(D_SG)
    eng.get_params(Pd, wd)
    eng.close()
    print("max |P - P_o|", np.abs(Pd - Po.swapaxes(1, 2)).max(), "max |w - w_o|",
          np.abs(wd - wo).max())
    np.testing.assert_allclose(Pd, Po.swapaxes(1, 2), rtol=0, atol=1e-10)
    np.testing.assert_allclose(wd, wo, rtol=0, atol=1e-10)


def test_psgd_adagrad_against_the_restated_step(oracle):
    """learning_rate='adagrad' on the first shape, weighted: the mean gradient of a minibatch
    from the oracle on its replicated rows (all penalties 0, unit step), the step from
    ``pairwise._adaptive_step``; parameters and accumulators."""
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.pairwise import _adaptive_step

    regname, k, degree, batch, G0 = "l1", 8, 2, 32, 1.0
    alpha, beta, gamma, eta0 = 1e-2, 1e-2, 0.2, 0.05
    X, y, idx, w, rows, rng = _psgd_problem()
    P0, w0, lams = _psgd_start(rng, k, 1, scale=0.3)   # gradients large enough to move the steps
    eng = HipEngine(0, "f64")
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "squared", regname, degree)
    eng.set_sample_weight(w)
    eng.psgd_set_adaptive(1, G0)
    P, wl = P0.copy(), w0.copy()                        # (n_orders, k, d)
    acc = (np.zeros((1, D_SG)), np.zeros(D_SG))
    it = 1
    for ep in range(2):
        sl_d, it = eng.psgd_epoch(degree, alpha, beta, gamma, eta0, "constant", 1.0, batch, idx,
                                  True, it)
        sl_r = 0.0
        for pos in range(0, N_SG, batch):
            rb = rows[pos:pos + batch]                  # B replicated rows = B visited rows
            Pc, wc = np.ascontiguousarray(P.swapaxes(1, 2)), wl.copy()
            sl, _ = oracle.psgd_epoch(Pc, wc, oracle.CSR(X[rb]), y[rb], lams, degree, 0.0, 0.0,
                                      0.0, regname, "squared",
                                      np.arange(rb.size, dtype=np.int32), True, 1.0, "constant",
                                      1.0, rb.size, 1)
            sl_r += sl
            gP = P - Pc.swapaxes(1, 2)                  # the mean gradient (B = 1 below)
            P, wl = _adaptive_step(P, wl, gP, wl - wc, 1, eta0, eta0, alpha, beta, gamma,
                                   regname, True, G0, acc)
        print("epoch", ep, "sum_loss", sl_d, sl_r)
        np.testing.assert_allclose(sl_d, sl_r, rtol=1e-11)
    assert it == 1 + 2 * (N_SG // batch)
    Pd, wd = np.empty_like(P0), np.empty(D_SG)
    eng.get_params(Pd, wd)
    aP, aw = eng.psgd_get_adaptive()
    eng.close()
    np.testing.assert_allclose(Pd, P, rtol=0, atol=1e-10)
    np.testing.assert_allclose(wd, wl, rtol=0, atol=1e-10)
    np.testing.assert_allclose(aP, acc[0], rtol=0, atol=1e-10)
    np.testing.assert_allclose(aw, acc[1], rtol=0, atol=1e-10)
    # the steps really differ per feature: an accumulator of 0.1 G0 shortens a step by 5 %, nine
    # orders of magnitude above the tolerances, and the features' accumulators spread widely
    assert acc[0].max() > 0.1 * G0 and acc[0].max() > 3 * acc[0].min()


def test_psgd_batch_of_one_and_zero_weight_batches():
    """batch_size=1: a weight still matters (the gradient is divided by the row count 1, not by
    the weight), and a zero-weight row's batch is a plain shrink step that advances ``it``."""
    from sparsepoly_amd.engine import HipEngine

    X, y, idx, w, rows, rng = _psgd_problem()
    P0, w0, lams = _psgd_start(rng, 8, 1)
    out = []
    for weights in (w, np.where(w > 0, 1.0, 0.0)):
        eng = HipEngine(0, "f64")
        eng.set_data(X, y)
        eng.set_params(P0, w0, lams)
        eng.configure("psgd", "squared", "l1", 2)
        eng.set_sample_weight(weights)
        sl, it = eng.psgd_epoch(2, 1e-2, 0.5, 0.003, 0.05, "optimal", 0.8, 1, idx, True, 1)
        assert it == 1 + N_SG and np.isfinite(sl)
        out.append(eng.get_params()[0])
        eng.close()
    assert np.all(np.isfinite(out[0])) and not np.array_equal(out[0], out[1])


# ------------------------------------------------- 4. estimators
def _small_problem(n=200, d=40, seed=3):
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(n, d, 5, seed=seed)
    X = sp.csr_matrix(X)
    w = np.random.RandomState(seed).randint(0, 4, size=n).astype(np.float64)
    return X, y, w


def _fit(est, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return est.fit(*args, **kw)


@pytest.mark.parametrize("kind", ["fm", "all_subsets"])
def test_estimator_equals_the_fit_on_replicated_rows(kind):
    """mean=True: the penalties scale with sum(w), which is the replicated row count"""
    from sparsepoly_amd import SparseAllSubsetsRegressor, SparseFactorizationMachineRegressor

    X, y, w = _small_problem()
    kw = dict(solver="pcd", schedule="exact", shuffle=False, mean=True, precision="f64",
              max_iter=5, tol=0, random_state=0, gamma=1e-3, beta=1e-3, n_components=4)
    if kind == "fm":  # (times sum(w) = 262: penalties under which squaredl12 keeps 80 % of P)
        kw.update(alpha=1e-4, beta=1e-4, gamma=1e-5)
    cls = SparseFactorizationMachineRegressor if kind == "fm" else SparseAllSubsetsRegressor
    a = _fit(cls(**kw), X, y, sample_weight=w)
    b = _fit(cls(**kw), *replicate_rows(X, y, w))
    assert a.sample_weight_sum_ == w.sum() and b.sample_weight_sum_ == float(int(w.sum()))
    print("max |P_a - P_b|", np.abs(a.P_ - b.P_).max())
    assert np.abs(a.P_).max() > 1e-3
    np.testing.assert_allclose(a.P_, b.P_, rtol=0, atol=P_ATOL["f64"])
    if kind == "fm":
        np.testing.assert_allclose(a.w_, b.w_, rtol=0, atol=P_ATOL["f64"])
    # ... and the scaling matters: without weights the fit is another one
    c = _fit(cls(**kw), X, y)
    assert c.sample_weight_sum_ == float(X.shape[0])
    assert np.abs(a.P_ - c.P_).max() > 100 * P_ATOL["f64"]


@pytest.mark.parametrize("solver", ["pcd", "pbcd", "psgd"])
def test_class_weight_balanced_is_the_explicit_vector(solver):
    from sparsepoly_amd import SparseFactorizationMachineClassifier

    X, y, _ = _small_problem()
    labels = np.where(y > np.quantile(y, 0.8), "pos", "neg")      # 1 : 4
    kw = dict(solver=solver, precision="f64", max_iter=3, tol=0, random_state=0, gamma=1e-3,
              beta=1e-3, alpha=1e-3, n_components=4, loss="logistic",
              regularizer="l21" if solver != "pcd" else "l1")
    if solver == "psgd":
        kw.update(eta0=0.05, learning_rate="constant", batch_size=16, tol=-1.0)
    a = SparseFactorizationMachineClassifier(**kw)
    a.class_weight = "balanced"
    _fit(a, X, labels)
    v = class_weight_vector("balanced", labels)
    b = _fit(SparseFactorizationMachineClassifier(**kw), X, labels, sample_weight=v)
    np.testing.assert_allclose(a.sample_weight_sum_, len(labels), rtol=1e-12)
    # (psgd sums a minibatch's gradient with atomics, in no fixed order: its own f64 tolerance)
    atol = 1e-10 if solver == "psgd" else 0.0
    np.testing.assert_allclose(a.P_, b.P_, rtol=0, atol=atol)
    np.testing.assert_allclose(a.w_, b.w_, rtol=0, atol=atol)
    c = _fit(SparseFactorizationMachineClassifier(**kw), X, labels)
    assert not np.array_equal(a.P_, c.P_)
    assert set(a.predict(X)) <= {"pos", "neg"}


def test_warm_start_session_drops_the_weights():
    """the kept device session of a weighted fit must not weigh the next, unweighted one"""
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    X, y, w = _small_problem()
    kw = dict(solver="pcd", precision="f64", max_iter=3, tol=0, random_state=0, gamma=1e-3,
              beta=1e-3, alpha=1e-3, n_components=4, warm_start=True)
    a = _fit(SparseFactorizationMachineRegressor(**kw), X, y, sample_weight=w)
    assert a._device_session is not None
    P1, w1, lams = a.P_.copy(), a.w_.copy(), a.lams_.copy()
    _fit(a, X, y)
    assert a.sample_weight_sum_ == float(X.shape[0])
    b = SparseFactorizationMachineRegressor(**kw)
    b.P_, b.w_, b.lams_ = P1.copy(), w1.copy(), lams
    _fit(b, X, y)
    a.release_device()
    b.release_device()
    np.testing.assert_array_equal(a.P_, b.P_)
    np.testing.assert_array_equal(a.w_, b.w_)


# ------------------------------------------------- 5. refusals
def test_estimator_refusals():
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.regularizer import L1

    class MyL1(L1):
        pass

    X, y, w = _small_problem()
    with pytest.raises(ValueError, match="distributed"):
        SparseFactorizationMachineRegressor(distributed=True).fit(X, y, sample_weight=w)
    est = SparseFactorizationMachineRegressor()
    est._REGULARIZERS = dict(est._REGULARIZERS, mine=MyL1)
    est.regularizer = "mine"
    with pytest.raises(ValueError, match="built-in"):
        est.fit(X, y, sample_weight=w)
    assert not hasattr(est, "P_")
    with pytest.raises(ValueError):
        SparseFactorizationMachineRegressor().fit(X, y, sample_weight=w[:-1])


def test_c_abi_refusals():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    X, y, w = _small_problem()
    n, d = X.shape
    eng = HipEngine(0, "f64")
    lib, h = eng._lib, eng._h

    def call(vec, count=None):
        a, p = _capi.f64(vec)
        return lib.spfm_set_sample_weight(h, p, a.shape[0] if count is None else count)

    assert call(w) == _capi.SPFM_ERR_INVALID                    # no data yet
    eng.set_data(X, y)
    assert call(w[:-1]) == _capi.SPFM_ERR_INVALID               # wrong n
    neg = w.copy()
    neg[3] = -1.0
    assert call(neg) == _capi.SPFM_ERR_INVALID
    nan = w.copy()
    nan[5] = np.nan
    assert call(nan) == _capi.SPFM_ERR_INVALID
    assert call(np.zeros(n)) == _capi.SPFM_ERR_INVALID          # all zero
    assert "zero" in lib.spfm_last_error(h).decode()
    assert not eng.sample_weight_set()
    assert call(w) == 0 and eng.sample_weight_set()
    # the triple epoch, the sharded epoch and the host-stepped epochs refuse a weighted handle
    rng = np.random.RandomState(0)
    eng.set_params(0.01 * rng.randn(1, 4, d), np.zeros(d), np.ones(4))
    eng.configure("psgd", "squared", "l1", 2)
    triples = np.array([[0, 1, 2]], dtype=np.int32)
    with pytest.raises(NotImplementedError, match="sample weights"):
        eng.psgd_pairs_epoch(2, 0.0, 0.0, 0.0, 0.1, "constant", 1.0, 1, triples, False, 1)
    with pytest.raises(NotImplementedError, match="sample weights"):
        eng.psgd_epoch(2, 0.0, 0.0, 0.0, 0.1, "constant", 1.0, 8,
                       np.arange(n, dtype=np.int32), False, 1, row_lo=0)
    eng.configure("pcd", "squared", "l1", 2)
    assert lib.spfm_host_epoch_begin(h, 0, 2) == _capi.SPFM_ERR_UNSUPPORTED
    # new data clears the weights
    eng.set_data(X, y)
    assert not eng.sample_weight_set() and eng.sample_weight_sum() == float(n)
    eng.close()


# ------------------------------------------------- 6. folds on one image
def test_folds_on_one_image():
    from sklearn.base import clone

    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.concurrent import fit_concurrently
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(400, 60, 5, seed=11)
    X = sp.csr_matrix(X)
    fold = np.arange(400) % 4
    masks = [(fold != f).astype(np.float64) for f in range(4)]
    base = SparseFactorizationMachineRegressor(solver="pcd", schedule="colored", max_iter=4, tol=0,
                                               random_state=0, gamma=1e-3, beta=1e-3, alpha=1e-3,
                                               n_components=4, precision="f32")
    ests = [clone(base) for _ in range(4)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fit_concurrently(ests, X, y, sample_weights=masks)
    assert sum(bool(e.shared_image_) for e in ests) == 3         # the followers
    for e, m in zip(ests, masks):
        solo = _fit(clone(base), X, y, sample_weight=m)
        assert e.sample_weight_sum_ == 300.0
        np.testing.assert_array_equal(e.P_, solo.P_)
        np.testing.assert_array_equal(e.w_, solo.w_)
    assert not np.array_equal(ests[0].P_, ests[1].P_)
    with pytest.raises(ValueError):
        fit_concurrently(ests, X, y, sample_weights=masks[:3])


def test_one_vs_rest_balanced():
    from sparsepoly_amd import SparseFactorizationMachineClassifier
    from sparsepoly_amd.multiclass import OneVsRestClassifier
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(300, 40, 5, seed=4)
    X = sp.csr_matrix(X)
    labels = np.digitize(y, np.quantile(y, [0.6, 0.9]))           # 3 classes, 6 : 3 : 1
    base = SparseFactorizationMachineClassifier(loss="logistic", max_iter=5, tol=0, random_state=0,
                                                gamma=1e-4, beta=1e-3, alpha=1e-3, n_components=4)
    ovr = OneVsRestClassifier(base)
    ovr.class_weight = "balanced"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ovr.fit(X, labels)
    assert all(e.class_weight == "balanced" for e in ovr.estimators_)
    assert all(abs(e.sample_weight_sum_ - 300.0) < 1e-9 for e in ovr.estimators_)
    pred = ovr.predict(X)
    assert pred.shape == (300,) and set(pred) <= {0, 1, 2}
    # member c is the solo binary fit with 'balanced' on its own one-against-the-rest target
    solo = SparseFactorizationMachineClassifier(**base.get_params())
    solo.class_weight = "balanced"
    _fit(solo, X, np.where(labels == 2, 1, -1))
    np.testing.assert_array_equal(ovr.estimators_[2].P_, solo.P_)
    ovr.release_device()
