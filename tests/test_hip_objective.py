"""``spfm_objective_terms`` / ``spfm_set_eval_csr`` / ``spfm_eval_loss`` and what the estimators
build on them, on the device.  Needs a real MI355X: ``pytest -m gpu``.

The device values are compared with the NumPy restatement of ``tests/test_objective_host.py``
(itself pinned to the reference's recorded ``eval`` values there).  Bounds: 1e-10 relative against
the fixture (the suite's oracle-versus-fixture bound); ``4 (d + k) max(degree, 1) 2^-53`` relative
against the float64 restatement -- all summands are non-negative, so each side's forward error is
at most its operation count times the unit round-off; counts are exact.

Trajectory tolerances are those of ``tests/test_hip_parity.py`` for the per-iteration loss sum
(``TRAJ_RTOL``: 1e-9 relative in f64 storage, 1e-5 in f32).
"""
import json
import pickle
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import golden_csr, load_golden
from test_objective_host import restate_bound, restate_terms, restate_terms_large  # noqa: F401

pytestmark = pytest.mark.gpu

COUNTS = ("nnz", "active_features", "active_components")
# (solver, regularizer) pairs spfm_configure accepts, and the degrees each takes
PAIRS = {"l1": "pcd", "squaredl12": "pcd", "omegati": "pcd", "l21": "pbcd", "squaredl21": "pbcd",
         "omegacs": "pbcd"}


def _engine(d, k, reg, top_degree, precision="f64", n_orders=1, options=None):
    """A handle with a one-row matrix (configure wants data), parameters to be set by the caller"""
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, precision)
    for key, val in (options or {}).items():
        eng.set_option(key, val)
    X = sp.csr_matrix((np.ones(1), (np.zeros(1, dtype=int), np.zeros(1, dtype=int))), shape=(1, d))
    eng.set_data(X, np.zeros(1))
    eng.set_params(np.zeros((n_orders, k, d)), np.zeros(d), np.ones(k))
    eng.configure(PAIRS[reg], "squared", reg, top_degree)
    return eng


def _close(got, want, rel):
    if np.isnan(want):
        return True  # nothing to compare like with like
    if np.isinf(want) or want == 0.0:
        return got == want
    return abs(got - want) <= rel * abs(want)


def _check(got, want, rel, what):
    assert not np.isnan(got["l2"]) and not np.isnan(got["omega"]), (what, got)
    for key in COUNTS:
        assert got[key] == want[key], (what, key, got, want)
    for key in ("l2", "omega"):
        assert _close(got[key], want[key], rel), (what, key, got[key], want[key])


# ------------------------------------------------------------------ 5. fixture parity
def test_fixture_parity():
    z = load_golden("g10_reg_eval.npz")
    blocks = [("P2", None, z["P2"].T)] + [("P3", q, z["P3"][q].T) for q in range(3)]

    def rec(key, q):
        return float(z[key]) if q is None else float(z[key][q])

    for name, q, P in blocks:
        k, d = P.shape
        for reg, key, degs in (("l1", "l1|%s", (2,)), ("l21", "l21|%s|t0", (2,)),
                               ("squaredl12", "squaredl12|%s|t1", (2,)),
                               ("squaredl21", "squaredl21|%s|t0", (2,)),
                               ("omegati", None, (2, 3, 4)), ("omegacs", None, (2, 3, 4))):
            eng = _engine(d, k, reg, max(degs))
            eng.set_params(P[None], np.zeros(d), np.ones(k))
            for deg in degs:
                got = eng.objective_terms(0, deg)
                want = restate_terms(P, reg, deg)
                if reg == "omegacs":   # the documented deviation: the prox cache, not eval
                    ref = want["omega"]
                    assert abs(ref - rec("omegacs|%s|deg%d" % (name, deg), q)) > 1e-3 * ref
                elif reg == "omegati":
                    ref = rec("omegati|%s|deg%d" % (name, deg), q)
                else:
                    ref = rec(key % name, q)
                np.testing.assert_allclose(got["omega"], ref, rtol=1e-10)
                np.testing.assert_allclose(got["l2"], want["l2"], rtol=1e-10)
                for c in COUNTS:
                    assert got[c] == want[c]
            if reg == "omegati" and q is None:
                got = eng.objective_terms(0, -1)
                np.testing.assert_allclose(got["omega"], float(z["omegati|P2|deg-1"]), rtol=1e-10)
            eng.close()
    # the three slices of P3 at degree -1: the fixture holds their sum
    tot = 0.0
    for q in range(3):
        P = z["P3"][q].T
        eng = _engine(P.shape[1], P.shape[0], "omegati", 2)
        eng.set_params(P[None], np.zeros(P.shape[1]), np.ones(P.shape[0]))
        tot += eng.objective_terms(0, -1)["omega"]
        eng.close()
    np.testing.assert_allclose(tot, float(z["omegati|P3|deg-1"]), rtol=1e-10)


# ------------------------------------------------------------------ 6. shape sweep
def _variants(rng, k, d):
    dense = rng.randn(k, d)
    holes = rng.randn(k, d)
    holes[rng.rand(k) < 0.4] = 0.0
    holes[:, rng.rand(d) < 0.5] = 0.0
    holes[rng.rand(k, d) < 0.3] = 0.0
    extreme = rng.randn(k, d)
    extreme[rng.rand(k, d) < 0.3] = 1e-160
    extreme[rng.rand(k, d) < 0.05] = -1e150
    return (("dense", dense), ("holes", holes), ("zero", np.zeros((k, d))), ("extreme", extreme))


def _wants(P):
    """restatement of every (regularizer, degree) of one block from ONE pass: the coefficients
    e_1..e_6 of a product truncated at t^6 are those of the product truncated lower"""
    from test_objective_host import esp_tree

    base = restate_terms(P, "l1", 2)
    A = np.abs(P)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        norms = np.sqrt((P * P).sum(axis=0))
        ti = esp_tree(A, 6).sum(axis=0)
        cs = esp_tree(norms[None], 6)[0]
        omega = {("l1", 2): A.sum(), ("l21", 2): norms.sum(),
                 ("squaredl12", 2): (A.sum(axis=1) ** 2).sum(), ("squaredl21", 2): norms.sum() ** 2}
    for deg in range(1, 7):
        omega[("omegati", deg)] = ti[deg]
        omega[("omegacs", deg)] = cs[deg]
    return {key: dict(base, omega=float(val)) for key, val in omega.items()}


@pytest.mark.parametrize("d", [1, 63, 64, 65, 4097, 100000])
def test_shape_sweep(d):
    rng = np.random.RandomState(d)
    for k in (1, 30, 31, 64, 65):
        engs = {reg: _engine(d, k, reg, 2 if reg.startswith("squared") else 6)
                for reg in PAIRS}
        for vname, P in _variants(rng, k, d):
            for eng in engs.values():
                eng.set_params(P[None], P[0], np.ones(k))
            for (reg, deg), want in _wants(P).items():
                _check(engs[reg].objective_terms(0, deg), want, restate_bound(k, d, deg),
                       (d, k, vname, reg, deg))
            tw = engs["l1"].objective_terms(-1, 1)
            ww = restate_terms(P[:1], "l1", 1)
            assert tw["nnz"] == ww["nnz"] and tw["omega"] == 0.0
            assert tw["active_features"] == 0 and tw["active_components"] == 0
            assert _close(tw["l2"], ww["l2"], restate_bound(1, d, 1))
        if d <= 4097:  # the all-subsets products overflow beyond (in the reference as well)
            P = 0.01 * rng.randn(k, d)
            P[:, ::5] = 0.0
            for reg in ("omegati", "omegacs", "l1"):
                engs[reg].set_params(P[None], np.zeros(d), np.ones(k))
                _check(engs[reg].objective_terms(0, -1), restate_terms(P, reg, -1),
                       restate_bound(k, d, 1), (d, k, "all-subsets", reg))
        for eng in engs.values():
            eng.close()


def test_errors():
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    with pytest.raises(ValueError):
        eng.objective_terms(0, 2)            # no parameters
    eng.close()
    eng = _engine(8, 2, "l1", 2)
    for deg in (0, 7, -2):
        with pytest.raises(NotImplementedError):
            eng.objective_terms(0, deg)
        with pytest.raises(ValueError):      # no held-out set yet
            eng.eval_loss(2, False, False)
    with pytest.raises(ValueError):
        eng.objective_terms(1, 2)
    with pytest.raises(ValueError):
        eng.set_eval_data(sp.csr_matrix((3, 9)), np.zeros(3))   # wrong d
    lib, h = eng._lib, eng._h
    from sparsepoly_amd import _capi

    ip = _capi.i64([0, 2])
    ji = _capi.i32([3, 1])                                      # unsorted
    dv = _capi.f64([1.0, 1.0])
    assert lib.spfm_set_eval_csr(h, 1, 8, ip[1], ji[1], dv[1], None) == _capi.SPFM_ERR_INVALID
    eng.set_eval_data(sp.csr_matrix((3, 8)))                    # no targets
    with pytest.raises(NotImplementedError):
        eng.eval_loss(7, False, False)
    eng.close()


# ------------------------------------------------------------------ problems for live fits
def _problem(n, d, per_row, seed):
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.randint(0, d, size=n * per_row)
    vals = rng.randn(n * per_row).astype(np.float32).astype(np.float64)
    X = sp.csr_matrix((vals, (rows, cols)), shape=(n, d))
    X.sum_duplicates()
    X.sort_indices()
    y = rng.randn(n).astype(np.float32).astype(np.float64)
    return X, y


class _Live(object):
    """One handle driven epoch by epoch like the estimators; `probe` is called between all
    epochs."""

    def __init__(self, X, y, solver, reg, degree, precision="f64", options=None, k=4,
                 schedule="colored", loss="squared"):
        from sparsepoly_amd.engine import HipEngine

        d = X.shape[1]
        self.solver, self.reg, self.degree, self.k = solver, reg, degree, k
        self.n_orders = 1 if degree == -1 else degree - 1
        eng = self.eng = HipEngine(0, precision)
        for key, val in (options or {}).items():
            eng.set_option(key, val)
        eng.set_data(X, y)
        self.P0 = 0.05 * np.random.RandomState(1).randn(self.n_orders, k, d)
        eng.set_params(self.P0, np.zeros(d), np.ones(k))
        eng.configure(solver, loss, reg, degree)
        self.lin = degree != -1
        eng.init_pred(degree, self.lin, degree == 3)
        eng.set_schedule(schedule, np.arange(d, dtype=np.int32))
        self.viol, self.flags = [], []

    def blocks(self):
        if self.degree == -1:
            return [(0, -1)]
        return [(self.degree - deg if deg != self.degree else 0, deg)
                for deg in list(range(2, self.degree)) + [self.degree]]

    def iterate(self, probe=None):
        eng, ic = self.eng, np.arange(self.k, dtype=np.int32)
        beta = 10.0 if self.solver == "pcd" else 1.0
        if self.lin:
            self.viol.append(eng.cd_linear_epoch(0.5))
            if probe:
                probe(self)
        for o, deg in self.blocks():
            eta = 1.0 if deg != -1 else 0.1
            if self.solver == "pcd":
                self.viol.append(eng.pcd_epoch(o, deg, beta, 1e-3, eta, ic))
            else:
                self.viol.append(eng.pbcd_epoch(o, deg, beta, 1e-3, eta))
            self.flags.append(tuple(eng.get_option(key) for key in (
                "persistent_active", "pbprb_active", "wide_active", "relax_steps",
                "persistent_fallbacks")))
            if probe:
                probe(self)

    def terms(self):
        return [self.eng.objective_terms(o, deg) for o, deg in self.blocks()]

    def check_against_params(self, what):
        before = self.eng.loss_sum()
        P, w = self.eng.get_params()
        k, d = P.shape[1:]
        for (o, deg), got in zip(self.blocks(), self.terms()):
            _check(got, restate_terms_large(P[o], self.reg, deg), restate_bound(k, d, deg),
                   (what, o, deg))
        tw = self.eng.objective_terms(-1, 1)
        assert tw["nnz"] == int((w != 0).sum())
        assert _close(tw["l2"], 0.5 * float((w * w).sum()), restate_bound(1, d, 1))
        assert self.eng.loss_sum() == before  # the loss term of the dict, bit for bit


LIVE = {
    "pcd_sql12": ("pcd", "squaredl12", 2),
    "pcd_omegati3": ("pcd", "omegati", 3),
    "pbcd_l21": ("pbcd", "l21", 2),
    "pbcd_omegacs3": ("pbcd", "omegacs", 3),
    "all_pcd": ("pcd", "omegati", -1),
}


# ------------------------------------------------------------------ 7. determinism
def test_determinism_and_group_options():
    X, y = _problem(3000, 400, 12, 3)
    seen = {}
    for opts in (None, {"prb_groups": 32}, {"pbprb_groups": 128}, {"co_tenants": 2}):
        for case in ("pcd_omegati3", "pbcd_omegacs3"):
            run = _Live(X, y, *LIVE[case], options=opts)
            # the same parameter image in every handle: the options may change the epochs'
            # summation order, the terms of one image may not depend on them
            a = run.terms() + [run.eng.objective_terms(-1, 1)]
            b = run.terms() + [run.eng.objective_terms(-1, 1)]
            assert pickle.dumps(a) == pickle.dumps(b)
            seen.setdefault(case, a)
            assert pickle.dumps(seen[case]) == pickle.dumps(a), (case, opts)
            run.iterate()
            a, b = run.terms(), run.terms()
            assert pickle.dumps(a) == pickle.dumps(b)
            run.eng.close()


# ------------------------------------------------------------------ 8. read-only
@pytest.mark.parametrize("case", sorted(LIVE))
def test_read_only(case):
    X, y = _problem(20000, 2000, 8, 7)
    Xv, yv = _problem(500, 2000, 8, 8)
    out = []
    for probing in (True, False):
        run = _Live(X, y, *LIVE[case], precision="f32")
        run.eng.set_eval_data(Xv, yv)
        args = (run.degree, run.lin, run.degree == 3)

        def probe(r):
            r.terms()
            r.eng.objective_terms(-1, 1)
            r.eng.eval_loss(*args, return_pred=True)

        for _ in range(3):
            run.iterate(probe if probing else None)
        P, w = run.eng.get_params()
        out.append((P, w, run.eng.get_y_pred(), np.array(run.viol), run.flags))
        run.eng.close()
    a, b = out
    for i in range(4):
        assert np.array_equal(a[i], b[i]), (case, i)
    assert a[4] == b[4]


# ------------------------------------------------------------------ 9. live layouts
ENGINES = {
    # name: (case, options, (persistent_active, pbprb_active) expected after the epochs,
    #        problem, schedule, extra check on the handle)
    "persistent_pcd": ("pcd_omegati3", None, (1, None), (3000, 400, 12, 3), "colored", None),
    "multi_kernel_pcd": ("pcd_omegati3", {"persistent": 0}, (0, None), (3000, 400, 12, 3),
                         "colored", None),
    "persistent_pcd_deg2": ("pcd_sql12", None, (1, None), (3000, 400, 12, 3), "colored", None),
    # steps of more than 64 columns: the wide pass (the problem of test_hip_recovery.py)
    "wide_pcd": ("pcd_sql12", {"wide_min_cols": 0}, (1, None), (6000, 3000, 4, 11), "colored",
                 "wide"),
    # the reference order, tiny steps: relaxed runs (the problem shape of test_hip_relax.py)
    "relaxed_pcd": ("pcd_sql12", None, (1, None), (10000, 2000, 10, 2), "exact", "relax"),
    "persistent_pbcd": ("pbcd_omegacs3", None, (None, 1), (3000, 400, 12, 3), "colored", None),
    "multi_kernel_pbcd": ("pbcd_l21", {"pbcd_persistent": 0}, (None, 0), (3000, 400, 12, 3),
                          "colored", None),
    "all_subsets_pcd": ("all_pcd", None, (1, None), (3000, 400, 12, 3), "colored", None),
}


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(ENGINES))
def test_live_layouts(name, precision):
    case, opts, (want_prb, want_pb), prob, schedule, extra = ENGINES[name]
    X, y = _problem(*prob)
    run = _Live(X, y, *LIVE[case], precision=precision, options=opts, schedule=schedule)
    run.check_against_params("initial")
    for _ in range(2):
        run.iterate()
        run.check_against_params(name)
    if want_prb is not None:
        assert run.eng.get_option("persistent_active") == want_prb
    if want_pb is not None:
        assert all(f[1] == want_pb for f in run.flags)
    assert run.eng.get_option("persistent_fallbacks") == 0
    if extra == "wide":
        assert run.eng.get_option("wide_active") == 1 and run.eng.get_option("relax_steps") == 0
    elif extra == "relax":
        strict, merged = run.eng.n_batches, run.eng.get_option("relax_steps")
        assert strict > 500 and 0 < merged < 0.4 * strict, (strict, merged)
    run.eng.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_live_layout_psgd(precision):
    from sparsepoly_amd.engine import HipEngine

    X, y = _problem(2000, 300, 10, 5)
    d, k = 300, 5
    eng = HipEngine(0, precision)
    eng.set_data(X, y)
    eng.set_params(0.05 * np.random.RandomState(2).randn(1, k, d), np.zeros(d), np.ones(k))
    eng.configure("psgd", "squared", "squaredl12", 2)
    it = 1
    for _ in range(2):
        _, it = eng.psgd_epoch(2, 1e-2, 0.1, 1e-3, 0.05, "optimal", 1.0, 64,
                               np.arange(2000, dtype=np.int32), True, it)
        got = eng.objective_terms(0, 2)
        P, w = eng.get_params()
        _check(got, restate_terms(P[0], "squaredl12", 2), restate_bound(k, d, 2), "psgd")
        again = eng.objective_terms(0, 2)   # get_params made the (k,d) image valid as well:
        assert again == got                 # the same bits from either layout
        tw = eng.objective_terms(-1, 1)
        assert tw["nnz"] == int((w != 0).sum()) and tw["nnz"] > 0
        assert _close(tw["l2"], 0.5 * float((w * w).sum()), restate_bound(1, d, 1))
    eng.close()


@pytest.mark.parametrize("case", ["pcd_omegati3", "pbcd_omegacs3"])
def test_terms_after_a_rolled_back_persistent_pass(case):
    X, y = _problem(3000, 400, 12, 3)
    run = _Live(X, y, *LIVE[case], options={"debug_spin_max": 4096})
    run.iterate()
    assert run.eng.get_option("persistent_fallbacks") == 0
    run.eng.cd_linear_epoch(0.5)
    run.eng.set_option("debug_drop_group", 1)
    o, deg = run.blocks()[0]
    if run.solver == "pcd":
        run.eng.pcd_epoch(o, deg, 10.0, 1e-3, 1.0, np.arange(run.k, dtype=np.int32))
    else:
        run.eng.pbcd_epoch(o, deg, 1.0, 1e-3, 1.0)
    assert run.eng.get_option("persistent_fallbacks") == 1
    run.check_against_params("rolled back")
    run.eng.close()


# ------------------------------------------------------------------ 11. held-out loss
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_held_out_loss(oracle, precision):
    from sparsepoly_amd.engine import HipEngine

    rng = np.random.RandomState(11)
    n, d, k = 700, 60, 5
    Xv, yv = _problem(n, d, 6, 12)
    Xv = sp.csr_matrix(Xv.toarray() * (rng.rand(n, 1) > 0.1))  # some empty rows
    Xv.eliminate_zeros()
    ypm = np.where(yv > 0, 1.0, -1.0)
    for degree in (2, 3, 4, 5, 6, -1):
        n_orders = 2 if degree == 3 else 1
        for loss in ("squared", "squared_hinge", "logistic"):
            eng = HipEngine(0, precision)
            Xt, yt = _problem(50, d, 4, 13)
            eng.set_data(Xt, yt if loss == "squared" else np.where(yt > 0, 1.0, -1.0))
            scale = 0.3 if degree != -1 else 0.05
            eng.set_params(scale * rng.randn(n_orders, k, d), 0.1 * rng.randn(d),
                           np.sign(rng.randn(k)))
            eng.configure("pcd", loss, "l1", degree)
            args = (degree, degree != -1, degree == 3)
            target = yv if loss == "squared" else ypm
            eng.set_eval_data(sp.csr_matrix((0, d)), np.zeros(0))          # an empty matrix
            assert eng.eval_loss(*args) == 0.0
            eng.set_eval_data(Xv, target)                                   # replaces it
            total, pred = eng.eval_loss(*args, return_pred=True)
            assert np.array_equal(pred, eng.predict(Xv, *args))
            want = oracle.loss_sum(loss, pred, target)
            assert abs(total - want) <= 4.0 * n * 2.0 ** -53 * abs(want), (degree, loss, total, want)
            assert eng.eval_loss(*args) == total
            eng.close()


# ------------------------------------------------------------------ 12. estimators
def _fm(cls=None, **kw):
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    base = dict(degree=2, n_components=4, solver="pcd", regularizer="squaredl12", alpha=0.1,
                beta=10.0, gamma=0.05, max_iter=4, tol=0, random_state=0, schedule="colored",
                precision="f64", n_calls=1, device=0)
    base.update(kw)
    return (cls or SparseFactorizationMachineRegressor)(**base)


def _fit(est, X, y):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return est.fit(X, y)


@pytest.mark.parametrize("solver,reg", [("pcd", "squaredl12"), ("pbcd", "omegacs")])
def test_estimator_with_monitor(solver, reg):
    from sparsepoly_amd.engine import SpfmError
    from sparsepoly_amd.monitor import Monitor

    X, y = _problem(400, 64, 6, 21)
    Xv, yv = _problem(100, 64, 6, 22)
    beta = 10.0 if solver == "pcd" else 1.0
    plain = _fit(_fm(solver=solver, regularizer=reg, beta=beta), X, y)
    mon = Monitor()
    est = _fm(solver=solver, regularizer=reg, beta=beta, callback=mon)
    est.set_validation(Xv, yv)
    _fit(est, X, y)
    assert len(mon.history) == est.n_iter_ + 1 == 4
    assert np.array_equal(est.P_, plain.P_) and np.array_equal(est.w_, plain.w_)
    assert est.n_iter_ == plain.n_iter_
    last = mon.history[-1]
    assert last["validation_loss"] == est.validation_loss_
    want = 0.5 * float(((est.predict(Xv) - yv) ** 2).sum())
    np.testing.assert_allclose(est.validation_loss_, want, rtol=1e-12)
    with pytest.raises(SpfmError, match="callback.*warm_start"):
        est.objective_terms()
    obj = est.objective(X, y)
    np.testing.assert_allclose(obj["objective"], last["objective"], rtol=1e-9)
    assert obj["nnz_P"] == last["nnz_P"] and obj["active_features"] == last["active_features"]
    P = est.P_[0]
    t = restate_terms(P, reg, 2)
    np.testing.assert_allclose(last["omega"][0], t["omega"], rtol=restate_bound(4, 64, 2))
    full = last["loss"] + 0.1 * last["l2_w"] + beta * last["l2_P"][0] + 0.05 * last["omega"][0]
    assert last["objective"] == full
    # a warm_start session keeps the terms available after fit
    warm = _fm(solver=solver, regularizer=reg, beta=beta, warm_start=True)
    _fit(warm, X, y)
    assert warm.objective_terms()["nnz_P"] == [int((warm.P_[0] != 0).sum())]
    warm.release_device()
    with pytest.raises(SpfmError):
        warm.objective_terms()


def test_plain_callback_still_receives_synced_params():
    X, y = _problem(400, 64, 6, 21)
    seen = []
    est = _fm(callback=lambda e: seen.append(e.P_.copy()) and None)
    _fit(est, X, y)
    assert len(seen) == 4 and np.array_equal(seen[-1], est.P_)
    assert not np.array_equal(seen[0], seen[-1])


# ------------------------------------------------------------------ 10. trajectory
TRAJ_RTOL = {"f64": 1e-9, "f32": 1e-5}   # tests/test_hip_parity.py: per-iteration loss sums


def _oracle_objectives(oracle, X, y, m, P0, lams, n_iter):
    """objective after each of the first n_iter iterations of the oracle's float64 run in the
    reference order: loss from its history, penalties by the restatement on its P, w"""
    out = []
    for it in range(1, n_iter + 1):
        fm = oracle.OracleFM(degree=m["degree"], loss=m["loss"], n_components=m["k"],
                             solver=m["solver"], regularizer=m["regularizer"], alpha=m["alpha"],
                             beta=m["beta"], gamma=m["gamma"], tol=0, fit_lower="explicit",
                             fit_linear=True, max_iter=it, eta0=1.0)
        fm.fit(X, y, P_init=P0, lams_init=lams)
        assert len(fm.history) == it
        obj = fm.history[-1][1] + m["alpha"] * 0.5 * float((fm.w_ * fm.w_).sum())
        for o in range(fm.P_.shape[0]):
            t = restate_terms(fm.P_[o], m["regularizer"], m["degree"] - o)
            obj += m["beta"] * t["l2"] + m["gamma"] * t["omega"]
        out.append(obj)
    return np.array(out)


def _device_objectives(X, y, m, P0, lams, n_iter, precision):
    from sparsepoly_amd.monitor import Monitor

    mon = Monitor()
    est = _fm(degree=m["degree"], n_components=m["k"], solver=m["solver"],
              regularizer=m["regularizer"], alpha=m["alpha"], beta=m["beta"], gamma=m["gamma"],
              max_iter=n_iter, eta0=1.0, schedule="exact", precision=precision, callback=mon,
              warm_start=True)
    est.P_, est.w_, est.lams_ = P0.copy(), np.zeros(X.shape[1]), lams.copy()
    _fit(est, X, y)
    est.release_device()
    assert len(mon.history) == n_iter
    return np.array([h["objective"] for h in mon.history])


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_trajectory_g2_config1(oracle, precision):
    """BASELINE config 1 (pcd + l1 + squared loss, degree 2, eta0 = 1): the objective of every
    iteration against the oracle's; in f64 it never rises -- first in the oracle, then on the
    device."""
    z = load_golden("g2_config1.npz")
    X, y = golden_csr(z), z["y"]
    m = dict(degree=2, loss="squared", k=4, solver="pcd", regularizer="l1", alpha=1.0, beta=1.0,
             gamma=1e-3)
    P0 = 0.01 * np.random.RandomState(0).randn(1, 4, X.shape[1])
    ref = _oracle_objectives(oracle, X, y, m, P0, np.ones(4), 6)
    assert all(b <= a for a, b in zip(ref, ref[1:])), ref
    got = _device_objectives(X, y, m, P0, np.ones(4), 6, precision)
    print("objective g2 %s: device %r oracle %r" % (precision, got.tolist(), ref.tolist()))
    np.testing.assert_allclose(got, ref, rtol=TRAJ_RTOL[precision])
    if precision == "f64":
        assert all(b <= a for a, b in zip(got, got[1:])), got


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_trajectory_pbcd(oracle, precision):
    """g3 case c4 (pbcd + omegacs, degree 2, k = 30): Omega by the prox cache's definition"""
    z = load_golden("g3_small_configs.npz")
    X, y = golden_csr(z), z["y"]
    m = json.loads(str(z["meta|c4|squared"]))
    P0, lams = z["P0|c4|squared"], z["lams|c4|squared"]
    ref = _oracle_objectives(oracle, X, y, m, P0, lams, 4)
    got = _device_objectives(X, y, m, P0, lams, 4, precision)
    print("objective c4 %s: device %r oracle %r" % (precision, got.tolist(), ref.tolist()))
    np.testing.assert_allclose(got, ref, rtol=TRAJ_RTOL[precision])


def test_fit_path_passes_the_validation_set_on():
    X, y = _problem(400, 64, 6, 24)
    Xv, yv = _problem(100, 64, 6, 25)
    gammas = [0.5, 0.05, 0.005]
    base = _fm()
    base.set_validation(Xv, yv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        path = base.fit_path(X, y, gamma=gammas)
    for g, e in zip(gammas, path):
        solo = _fm(gamma=g)
        solo.set_validation(Xv, yv)
        _fit(solo, X, y)
        assert e.validation_loss_ == solo.validation_loss_


def test_classifier_labels_go_through_the_binarizer():
    from sparsepoly_amd import SparseFactorizationMachineClassifier
    from sparsepoly_amd.monitor import Monitor

    X, y = _problem(400, 64, 6, 26)
    Xv, yv = _problem(100, 64, 6, 27)
    lab, labv = np.where(y > 0, 7, 3), np.where(yv > 0, 7, 3)
    mon = Monitor()
    est = _fm(SparseFactorizationMachineClassifier, loss="squared_hinge", callback=mon)
    est.set_validation(Xv, labv)
    _fit(est, X, lab)
    z = 1.0 - est.decision_function(Xv) * np.where(labv == 7, 1.0, -1.0)
    np.testing.assert_allclose(est.validation_loss_, float((np.maximum(z, 0) ** 2).sum()),
                               rtol=1e-12)
    np.testing.assert_allclose(est.objective(X, lab)["objective"], mon.history[-1]["objective"],
                               rtol=1e-9)


@pytest.mark.parametrize("solver,reg", [("pcd", "omegati"), ("pbcd", "omegacs")])
def test_all_subsets_estimator(solver, reg):
    from sparsepoly_amd import SparseAllSubsetsRegressor
    from sparsepoly_amd.monitor import Monitor

    X, y = _problem(400, 64, 6, 28)
    Xv, yv = _problem(100, 64, 6, 29)
    kw = dict(n_components=4, solver=solver, regularizer=reg, beta=1.0, gamma=1e-3, max_iter=3,
              tol=0, random_state=0, precision="f64", n_calls=1, device=0)
    plain = _fit(SparseAllSubsetsRegressor(**kw), X, y)
    mon = Monitor()
    est = SparseAllSubsetsRegressor(callback=mon, **kw)
    est.set_validation(Xv, yv)
    _fit(est, X, y)
    assert len(mon.history) == 3 and np.array_equal(est.P_, plain.P_)
    last = mon.history[-1]
    t = restate_terms(est.P_, reg, -1)
    np.testing.assert_allclose(last["omega"][0], t["omega"], rtol=restate_bound(4, 64, 1))
    assert last["nnz_P"] == [t["nnz"]] and last["nnz_w"] == 0
    assert last["validation_loss"] == est.validation_loss_
    np.testing.assert_allclose(est.objective(X, y)["objective"], last["objective"], rtol=1e-9)
