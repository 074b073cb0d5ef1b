"""Fold-in of new columns (``sparsepoly_amd/foldin.py``) without a device: the affine identity the
design rests on, the restated Newton iteration on every case the device tests use, the symbols,
``extend_features`` and the argument errors.  ``tests/test_hip_foldin.py`` imports its cases from
here, so that no device case is skipped or left unconverged by its data."""
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from sklearn.utils.validation import NotFittedError
from test_explain_host import COMBOS, model_output, rows_matrix
from test_ranking_host import abs_model, all_subsets, fm

D = 800
LENGTHS = [1, 2, 63, 64, 65, 130]        # 1: the row is the target entry alone
ROWS_PER_COLUMN = [0, 1, 3, 70, 300]     # below R, above a wave, several chunks of the solve
TARGETS = np.array([200, 300, 400, 500, 600])
ALPHA, BETA = 0.7, 1.3
# (degree, fit_lower, fit_linear, k, loss, precision)
CASES = [
    (2, "explicit", True, 30, "squared", "f64"),
    (2, "explicit", False, 1, "squared", "f32"),
    (2, None, True, 64, "logistic", "f32"),
    (2, "explicit", True, 65, "squared_hinge", "f64"),
    (3, "explicit", True, 5, "logistic", "f64"),
    (3, "explicit", False, 64, "squared", "f32"),      # R = 128, the cap
    (3, "explicit", True, 30, "squared_hinge", "f32"),
    (4, "augment", True, 30, "logistic", "f32"),
    (4, "augment", False, 5, "squared", "f64"),
    (6, "explicit", True, 30, "squared", "f32"),       # orders 1..4 of P_ are not summed
    (6, None, False, 65, "logistic", "f64"),
]


def case_id(spec):
    return "-".join(str(v) for v in spec)


def estimator(degree, fit_lower, lin, k, loss, precision="f64", d=D, seed=0):
    """``fm`` with parameters small enough for rows of 130 entries at degree 6, of the class the
    loss belongs to"""
    from sklearn.preprocessing import LabelBinarizer
    from sparsepoly_amd import SparseFactorizationMachineClassifier

    cls = None if loss == "squared" else SparseFactorizationMachineClassifier
    est = fm(degree, k, d, fit_lower, lin, seed=seed, cls=cls)
    est.P_ *= 0.2
    est.w_ *= 0.5
    est.precision = precision
    if cls is not None:
        est.loss = loss
        est.label_binarizer_ = LabelBinarizer(pos_label=1, neg_label=-1).fit([-1, 1])
    est.alpha, est.beta = ALPHA, BETA
    return est


def target_rows(d=D, targets=TARGETS, rows_per_column=ROWS_PER_COLUMN, lengths=LENGTHS, seed=0,
                n_ignored=4):
    """CSR rows (values exact in float32): column ``targets[q]`` is stored by
    ``rows_per_column[q]`` rows whose lengths cycle through ``lengths`` and whose target entry
    stands first, in the middle or last in turn; ``n_ignored`` rows store no target.  The rows
    are shuffled."""
    rng = np.random.RandomState(seed + 7000)
    free = np.setdiff1d(np.arange(d), targets)
    rows, u = [], 0
    for j, cnt in zip(targets, rows_per_column):
        below, above = free[free < j], free[free > j]
        for _ in range(cnt):
            m = lengths[u % len(lengths)] - 1
            where = (u // len(lengths)) % 3
            u += 1
            n_below = min(max((0, m // 2, m)[where], m - above.size), below.size)
            others = np.concatenate([rng.choice(below, n_below, replace=False),
                                     rng.choice(above, m - n_below, replace=False)])
            rows.append(np.sort(np.concatenate([others, [j]])))
    for _ in range(n_ignored):
        rows.append(np.sort(rng.choice(free, 5, replace=False)))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = rng.randn(idx.size).astype(np.float32).astype(np.float64)
    data[data == 0] = 1.0
    return sp.csr_matrix((data, idx, indptr), shape=(len(rows), d))


def targets_for(est, n, seed=0):
    rng = np.random.RandomState(seed + 8000)
    if hasattr(est, "decision_function"):
        return np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    return rng.randn(n)


def build_case(spec):
    """-> (est, X, y) of a device case"""
    seed = CASES.index(spec)
    est = estimator(*spec, seed=seed)
    X = target_rows(seed=seed)
    return est, X, targets_for(est, X.shape[0], seed)


# ---------------------------------------------------------------- 1. the design
def _design_specs():
    from sparsepoly_amd import SparseFactorizationMachineClassifier

    out = [pytest.param((None, dg, fl, lin), id="reg-%d-%s-%d" % (dg, fl, lin))
           for dg, fl, lin in COMBOS]
    out.append(pytest.param((SparseFactorizationMachineClassifier, 3, "explicit", True),
                            id="classifier-3-explicit-1"))
    return out


@pytest.mark.parametrize("spec", _design_specs())
def test_output_is_affine_in_the_target_column(spec):
    """the model's output on rows whose column j is set to theta equals c + Z theta: theta = 0,
    every unit vector and a random theta; pins the skipped entry, the 'augment' table and the
    explicit degree-3 second block"""
    from sklearn.preprocessing import LabelBinarizer
    from sparsepoly_amd.foldin import restate_fold_in

    cls, degree, fl, lin = spec
    d, k = 12, 3
    est = fm(degree, k, d, fl, lin, seed=50 + degree, cls=cls)
    if cls is not None:
        est.label_binarizer_ = LabelBinarizer(pos_label=1, neg_label=-1).fit([-1, 1])
    targets = np.array([3, 7])
    X = target_rows(d, targets, [3, 4], [1, 2, 5, 9], seed=degree, n_ignored=2)
    y = targets_for(est, X.shape[0])
    res = restate_fold_in(est, X, y, targets, alpha=1.0, beta=1.0)
    pr = res.problem
    rng = np.random.RandomState(degree)
    thetas = [np.zeros(pr.R)] + list(np.eye(pr.R)) + [rng.randn(pr.R)]
    assert res.n_rows.tolist() == [3, 4] and pr.ignored == 2
    V = X.toarray()
    for q, j in enumerate(targets):
        rows, Z, c = res.rows[q], res.Z[q], res.c[q]
        assert Z.shape == (len(rows), pr.R) and (np.diff(rows) > 0).all()
        for theta in thetas:
            moved = _with_column(est, pr, j, theta)
            want = model_output(moved, V[rows])
            # the magnitudes a value is made of: the output of the model of magnitudes
            S = model_output(abs_model(moved), np.abs(V[rows]))
            assert (np.abs(c + Z @ theta - want) <= 1e-12 * S).all(), (q, theta)


def _with_column(est, pr, j, theta):
    """a copy of ``est`` whose column j (a feature of X) holds theta"""
    import copy

    moved = copy.copy(est)
    moved.P_, moved.w_ = est.P_.copy(), est.w_.copy()
    stored, lin = pr.real[j], int(pr.lin)
    if lin:
        moved.w_[stored] = theta[0]
    for q, (o, _) in enumerate(pr.blocks):
        moved.P_[o, :, stored] = theta[lin + q * pr.k:lin + (q + 1) * pr.k]
    return moved


# ---------------------------------------------------------------- 2. the restated Newton
@pytest.mark.parametrize("spec", CASES, ids=case_id)
def test_restated_newton_converges_on_every_device_case(spec):
    from sparsepoly_amd.foldin import objective_parts, restate_fold_in

    est, X, y = build_case(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = restate_fold_in(est, X, y, TARGETS, max_iter=50, tol=1e-8)
    assert res.n_rows.tolist() == ROWS_PER_COLUMN
    assert res.converged.all() and (res.n_iter <= 50).all()
    assert (res.objective_after <= res.objective_before).all()
    pr = res.problem
    for q in range(len(TARGETS)):
        Z, c, yq = res.Z[q], res.c[q], pr.y[res.rows[q]]
        g0 = np.abs(objective_parts(pr.loss, Z, c, yq, res.lam, np.zeros(pr.R))[1]).max()
        g1 = np.abs(objective_parts(pr.loss, Z, c, yq, res.lam, res.theta[q])[1]).max()
        assert g1 <= 1e-8 * g0 and g1 == res.grad_norm[q]
        if ROWS_PER_COLUMN[q] == 0:
            assert (res.theta[q] == 0).all() and res.n_iter[q] == 0
        if spec[4] == "squared":
            assert res.n_iter[q] <= 2
            want = np.linalg.solve(Z.T @ Z + np.diag(res.lam), Z.T @ (yq - c))
            assert np.abs(res.theta[q] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    # the returned parameter blocks hold theta, the orders outside the blocks the estimator's
    stored, lin = pr.real[TARGETS], int(pr.lin)
    touched = [o for o, _ in pr.blocks]
    for o in range(est.P_.shape[0]):
        if o in touched:
            q = touched.index(o)
            assert (res.P[o] == res.theta[:, lin + q * pr.k:lin + (q + 1) * pr.k].T).all()
        else:
            assert (res.P[o] == est.P_[o][:, stored]).all()
    assert (res.w == (res.theta[:, 0] if lin else est.w_[stored])).all()


def test_wide_restatement_agrees_with_the_double_one():
    from sparsepoly_amd.foldin import restate_fold_in

    est, X, y = build_case(CASES[4])
    a = restate_fold_in(est, X, y, TARGETS)
    b = restate_fold_in(est, X, y, TARGETS, wide=True)
    assert b.theta.dtype == np.longdouble and b.Z[3].dtype == np.longdouble
    assert np.abs(a.theta - b.theta).max() <= 1e-7 * np.abs(b.theta).max()


# ---------------------------------------------------------------- 3. symbols
def test_header_capi_and_library_agree_on_the_new_symbols():
    from sparsepoly_amd import _capi

    names = ("spfm_foldin_csr", "spfm_foldin_set_partition", "spfm_foldin_info")
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS
    assert re.search(r"#define SPFM_FOLDIN_MAX_UNKNOWNS %d\b" % _capi.FOLDIN_MAX_UNKNOWNS, header)
    lib = _capi.load()
    for name in names:
        assert hasattr(lib, name), name


# ---------------------------------------------------------------- 4. extend_features
@pytest.mark.parametrize("degree,fl,lin", [(2, "explicit", True), (3, "explicit", False),
                                           (4, "augment", True), (3, "augment", False)])
def test_extend_features_inserts_zero_columns_after_the_last_real_one(degree, fl, lin):
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.explain import _columns

    d = 9
    est = fm(degree, 3, d, fl, lin, seed=3)
    P0, w0 = est.P_.copy(), est.w_.copy()
    real0, dummy0 = _columns(est, d)
    new = est.extend_features(4)
    assert new.tolist() == [9, 10, 11, 12]
    real, dummy = _columns(est, d + 4)
    assert est.P_.shape == (P0.shape[0], 3, P0.shape[2] + 4) and est.w_.shape == (w0.size + 4,)
    assert (est.P_[:, :, real[:d]] == P0[:, :, real0]).all() and (est.w_[real[:d]] == w0[real0]).all()
    assert (est.P_[:, :, dummy] == P0[:, :, dummy0]).all() and (est.w_[dummy] == w0[dummy0]).all()
    assert (est.P_[:, :, real[d:]] == 0).all() and (est.w_[real[d:]] == 0).all()
    # the old features' outputs are what they were
    X = rows_matrix([0, 2, 5], d, seed=1)
    wide = sp.hstack([X, sp.csr_matrix((3, 4))]).tocsr()
    old = fm(degree, 3, d, fl, lin, seed=3)
    np.testing.assert_allclose(model_output(est, wide.toarray()), model_output(old, X.toarray()),
                               rtol=1e-13, atol=1e-13)  # (a matrix product of another width)
    assert est.extend_features(0).size == 0
    with pytest.raises(NotFittedError):
        SparseFactorizationMachineRegressor().extend_features(1)
    with pytest.raises(ValueError, match="n_new"):
        est.extend_features(-1)


# ---------------------------------------------------------------- 5. argument errors
def test_argument_errors_come_before_any_device_use(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRegressor, engine
    from sparsepoly_amd.foldin import restate_fold_in

    def no_device(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", no_device)
    X = target_rows(20, np.array([3, 7]), [2, 3], [1, 2, 4], n_ignored=1)
    y = np.arange(X.shape[0], dtype=np.double)
    two = sp.csr_matrix(np.array([[0, 0, 0, 1.0, 0, 0, 0, 2.0] + [0] * 12, [1.0] * 3 + [0] * 17]))
    for est in (estimator(2, "explicit", True, 3, "squared", d=20),
                estimator(4, "augment", True, 3, "logistic", d=20)):
        yy = np.where(y % 2 == 0, -1.0, 1.0) if hasattr(est, "decision_function") else y
        for call in (est.fold_in, lambda *a, **k: restate_fold_in(est, *a, **k)):
            with pytest.raises(ValueError, match="features"):
                call(X[:, :19], yy, [3])
            with pytest.raises(ValueError, match="row 0 stores two target columns"):
                call(two, yy[:2], [3, 7])
            with pytest.raises(ValueError, match="listed twice"):
                call(X, yy, [3, 3])
            for bad in ([20], [-1]):
                with pytest.raises(ValueError, match="outside"):
                    call(X, yy, bad)
            with pytest.raises(ValueError, match="beta must be > 0"):
                call(X, yy, [3], beta=0.0)
            with pytest.raises(ValueError, match="alpha must be > 0"):
                call(X, yy, [3], alpha=-1.0)
            for bad in (0, 2.5):
                with pytest.raises(ValueError, match="max_iter"):
                    call(X, yy, [3], max_iter=bad)
            for bad in (-1e-3, np.inf, np.nan):
                with pytest.raises(ValueError, match="tol must be"):
                    call(X, yy, [3], tol=bad)
            with pytest.raises(ValueError, match="targets"):
                call(X, yy[:-1], [3])
    # no linear term: alpha is not looked at
    assert restate_fold_in(estimator(2, None, False, 3, "squared", d=20), X, y, [3],
                           alpha=0.0).converged.all()
    with pytest.raises(ValueError, match="exceed the cap"):
        estimator(3, "explicit", True, 64, "squared", d=20).fold_in(X, y, [3])
    unfitted = SparseFactorizationMachineRegressor()
    for call in (lambda: unfitted.fold_in(X, y, [3]), lambda: restate_fold_in(unfitted, X, y, [3])):
        with pytest.raises(NotFittedError):
            call()
    # reaching the device is the only thing left to go wrong for good arguments
    with pytest.raises(AssertionError, match="device handle"):
        estimator(2, "explicit", True, 3, "squared", d=20).fold_in(X, y, [3, 7])


def test_all_subsets_estimators_do_not_fold_in():
    est = all_subsets(3, 8)
    for name in ("fold_in", "extend_features"):
        assert not hasattr(est, name)


def test_inputs_are_left_alone():
    from sparsepoly_amd.foldin import restate_fold_in

    est = estimator(2, "explicit", True, 3, "squared", d=20)
    X = target_rows(20, np.array([3, 7]), [2, 3], [1, 2, 4], n_ignored=1)
    y = np.arange(X.shape[0], dtype=np.double)
    keep = X.copy(), y.copy(), est.P_.copy(), est.w_.copy()
    restate_fold_in(est, X, y, [7, 3])
    assert (X != keep[0]).nnz == 0 and (y == keep[1]).all()
    assert (est.P_ == keep[2]).all() and (est.w_ == keep[3]).all()
