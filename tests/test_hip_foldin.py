"""``spfm_foldin_*`` and what ``sparsepoly_amd.foldin`` builds on them, on the device.  Needs a
real MI355X: ``pytest -m gpu``.  The cases are those of ``tests/test_foldin_host.py``, where the
restated Newton iteration is held to converge on every one of them.

A device result ``theta`` is judged by the gradient of ``F_j`` at it, formed in ``longdouble`` by
the restatement (``restate_fold_in(..., wide=True)``):

    |grad F_j(theta)|_r <= tol max|grad F_j(0)| + (N + 2) 2^-53 S_r
    S_r = ((|Z|' D |Z| + Lambda) |theta| + |Z|' |l'|)_r,      D = diag(l'')

``|Z|`` from the model of magnitudes.  The device stops when ITS gradient meets the criterion; the
second term is what its gradient can differ from the exact one by.  ``N`` counts the roundings a
term of ``S_r`` goes through in ``foldin_design_kernel`` and ``foldin_solve_kernel``
(``csrc/spfm_foldin.hip.h``), and comes from no device run.  With ``n_i`` the stored entries of
the longest row of the column, ``n_j`` its rows, ``M`` the degree:
  * a design entry ``z_ir``: inside ``A^{t-1}`` one rounding per factor ``p x``, one per
    multiplication by it, one per addition of the recurrence, of which a row has ``n_i``:
    ``n_i + 2 (M - 1)``; the product with ``c[s][t]`` and the sum over ``t``: ``M + 1``; the
    products with ``lams_s`` (exact) and ``x_ij``: 1; ``fit_lower='augment'``: ``c[s][t]`` is the
    host's sum of products of at most ``M - 1`` dummy parameters, ``2 (M - 1)``; together at most
    ``n_i + 5 M - 2``;
  * a term ``|z_ir| |l'_i|``: ``z_ir``, the evaluation of ``l'`` from the margin (logistic: the
    product ``p y``, ``exp``, the addition, the division: 6 with a 2-ulp ``exp``), the product,
    the ``n_j`` additions over the rows and the addition of ``Lambda theta``:
    ``n_i + 5 M + 6 + n_j``;
  * a term ``|z_ir| l''_i |z_ir'| |theta_r'|`` -- how a rounding of the margin reaches ``l'``:
    ``z_ir'``, its product with ``theta_r'``, the lane sums (``ceil(R / 64)`` additions), the
    butterfly (6) and the addition of ``c_i``; then ``z_ir``, the product and the sums as above:
    ``2 n_i + 10 M + ceil(R / 64) + 6 + n_j``.
So ``N = 2 n_i + 10 M + ceil(R / 64) + 6 + n_j``; the 2 covers the second-order terms, the
``longdouble`` reference and the relative error of the device's ``max|grad F_j(0)|``.  (The
rounding of ``c_i`` itself has no term in ``S_r``; it enters like a rounding of the margin.)
Then, ``F_j`` being ``min(alpha, beta)``-strongly convex,
``|theta - theta*|_2 <= (|grad F(theta)|_2 + |grad F(theta*)|_2) / min(alpha, beta)`` against
the restatement's ``theta*``.  Each case prints its largest error as a fraction of its bound
before asserting.

The output identity uses the rounding bound of ``anova_predict_kernel`` as
``tests/test_hip_pairs.py`` has it: ``N_pred = n_i + n_dummy + 2 M + 2 + 6 + lower + 2`` roundings
against the output of the model of magnitudes.
"""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from test_explain_host import model_output
from test_foldin_host import (ALPHA, BETA, CASES, ROWS_PER_COLUMN, TARGETS, build_case, case_id,
                              estimator, target_rows, targets_for)
from test_ranking_host import abs_model

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CLEAR = 1e-9
TOL = 1e-8
LD = np.longdouble


def _reference(est, X, y, cols):
    """the wide restatement and the design of the model of magnitudes, NumPy only"""
    from sparsepoly_amd.foldin import _problem, restate_design, restate_fold_in

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ref = restate_fold_in(est, X, y, cols, tol=TOL, wide=True)
    assert ref.converged.all()
    mag = restate_design(_problem(abs_model(est), abs(X), y, cols, None, None, 50, TOL, LD), LD)
    return ref, mag


def _check_theta(est, ref, mag, theta, what):
    """the componentwise gradient bound and the distance to theta*"""
    from sparsepoly_amd.foldin import loss_terms, objective_parts

    pr = ref.problem
    degree = est.degree
    worst_g = worst_d = 0.0
    for q in range(len(ref.rows)):
        Z, c, yq = ref.Z[q], ref.c[q], pr.y[ref.rows[q]].astype(LD)
        th = theta[q].astype(LD)
        g = objective_parts(pr.loss, Z, c, yq, ref.lam, th)[1]
        g0 = np.abs(objective_parts(pr.loss, Z, c, yq, ref.lam, 0 * th)[1]).max(initial=0)
        _, d1, d2 = loss_terms(pr.loss, c + Z @ th, yq)
        aZ = mag[q][1]
        S = aZ.T @ (d2 * (aZ @ np.abs(th))) + ref.lam * np.abs(th) + aZ.T @ np.abs(d1)
        n_j = len(ref.rows[q])
        n_i = int(np.diff(pr.Xc.indptr)[ref.rows[q]].max(initial=0))
        N = 2 * n_i + 10 * degree + -(-pr.R // 64) + 6 + n_j
        bound = TOL * g0 + (N + 2) * U * S
        ok = bound > 0
        worst_g = max(worst_g, float((np.abs(g)[ok] / bound[ok]).max(initial=0.0)))
        assert (np.abs(g) <= bound).all(), (what, q, worst_g)
        gs = objective_parts(pr.loss, Z, c, yq, ref.lam, ref.theta[q])[1]
        dist = np.sqrt(((th - ref.theta[q]) ** 2).sum())
        dbound = (np.sqrt((g ** 2).sum()) + np.sqrt((gs ** 2).sum())) / min(pr.alpha, pr.beta)
        if dbound > 0:
            worst_d = max(worst_d, float(dist / dbound))
        assert dist <= dbound, (what, q, float(dist), float(dbound))
    print("%s: largest gradient %.3g of its bound, largest distance %.3g of its bound"
          % (what, worst_g, worst_d))


# ---------------------------------------------------------------- 1. values, output identity
@pytest.mark.parametrize("spec", CASES, ids=case_id)
def test_values_and_output_identity(spec):
    est, X, y = build_case(spec)
    ref, mag = _reference(est, X, y, TARGETS)
    pr = ref.problem
    P0, w0 = est.P_.copy(), est.w_.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a ConvergenceWarning fails the case
        res = est.fold_in(X, y, TARGETS, tol=TOL)
    assert (est.P_ == P0).all() and (est.w_ == w0).all()  # update=False: read-only
    assert res.theta.shape == (len(TARGETS), pr.R) and res.theta.dtype == np.float64
    assert res.n_rows.tolist() == ROWS_PER_COLUMN and res.converged.all()
    assert res.info["ignored_rows"] == pr.ignored == 4 and res.info["groups"] == 1
    assert (res.objective_after <= res.objective_before).all()
    assert (res.theta[0] == 0).all() and res.n_iter[0] == 0
    if spec[4] == "squared":
        assert (res.n_iter <= 2).all()
    _check_theta(est, ref, mag, res.theta, case_id(spec))
    for name in ("objective_before", "objective_after"):
        np.testing.assert_allclose(getattr(res, name), getattr(ref, name).astype(np.double),
                                   rtol=1e-6, atol=1e-9)
    # update=True: the same numbers, now in P_ / w_, and the model's output is c + Z theta
    again = est.fold_in(X, y, TARGETS, tol=TOL, update=True)
    assert (again.theta == res.theta).all()
    stored, lin = pr.real[TARGETS], int(pr.lin)
    assert (est.P_[:, :, stored] == res.P).all() and (est.w_[stored] == res.w).all()
    for o in set(range(est.P_.shape[0])) - {o for o, _ in pr.blocks}:
        assert (est.P_[o] == P0[o]).all()
    keep = np.setdiff1d(np.arange(est.P_.shape[2]), stored)
    assert (est.P_[:, :, keep] == P0[:, :, keep]).all() and (est.w_[keep] == w0[keep]).all()
    rows = np.concatenate(ref.rows)
    want = np.concatenate([ref.c[q] + ref.Z[q] @ res.theta[q].astype(LD)
                           for q in range(len(TARGETS))])
    Xr = X[rows]
    got = est.decision_function(Xr) if hasattr(est, "decision_function") else est.predict(Xr)
    n_dummy = est.P_.shape[2] - X.shape[1]
    N_pred = np.diff(Xr.indptr) + n_dummy + 2 * est.degree + 2 + 6 + len(pr.blocks) - 1 + 2
    bound = (N_pred + 2) * U * model_output(abs_model(est), np.abs(Xr.toarray()))
    ok = bound > 0  # (a row that is its target entry alone may have no term at all)
    frac = float((np.abs(got - want)[ok] / bound[ok]).max())
    print("output identity: largest error %.3g of its bound" % frac)
    assert (np.abs(got - want) <= bound).all(), frac


# ---------------------------------------------------------------- 2. bit-exact invariance
@pytest.mark.parametrize("spec", [CASES[2], CASES[5], CASES[7]], ids=case_id)
def test_bits_depend_on_a_columns_own_rows_alone(spec):
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.foldin import _problem, run

    est, X, y = build_case(spec)
    whole = est.fold_in(X, y, TARGETS, tol=TOL)
    # one call per column
    for q, j in enumerate(TARGETS):
        one = est.fold_in(X, y, [j], tol=TOL)
        assert (one.theta[0] == whole.theta[q]).all(), j
        assert one.n_iter[0] == whole.n_iter[q] and one.grad_norm[0] == whole.grad_norm[q]
        assert one.info["ignored_rows"] == X.shape[0] - ROWS_PER_COLUMN[q]
    # another order of the columns
    perm = [3, 0, 4, 2, 1]
    other = est.fold_in(X, y, TARGETS[perm], tol=TOL)
    assert (other.theta == whole.theta[perm]).all()
    # 1, 2 and many groups
    pr = _problem(est, X, y, TARGETS, None, None, 50, TOL)
    eng = HipEngine(0, est.precision)
    try:
        eng.set_params(pr.P, pr.w, pr.lams)
        # (a group takes whole columns, in the caller's order, while their rows fit)
        for max_rows, groups in ((0, 1), (10 ** 6, 1), (300, 2), (70, 3), (1, 4)):
            eng.foldin_set_partition(max_rows)
            out = run(eng, pr)
            info = eng.foldin_info()
            assert info["groups"] == groups and info["max_rows"] == max_rows, (max_rows, info)
            for name in ("theta", "n_iter", "grad_norm", "obj0", "obj1"):
                assert (out[name] == getattr(whole, {"obj0": "objective_before",
                                                     "obj1": "objective_after"}.get(name, name))
                        ).all(), (max_rows, name)
        assert info["scratch_kib"] > 0 and info["device_ms"] > 0
        with pytest.raises(ValueError, match="max_rows"):
            eng.foldin_set_partition(-1)
    finally:
        eng.close()
    # what the target columns hold is not read
    rng = np.random.RandomState(1)
    stored = pr.real[TARGETS]
    est.P_[:, :, stored] = rng.randn(*est.P_[:, :, stored].shape) * 1e3
    est.w_[stored] = rng.randn(len(stored)) * 1e3
    moved = est.fold_in(X, y, TARGETS, tol=TOL)
    assert (moved.theta == whole.theta).all()


# ---------------------------------------------------------------- 3. end to end
def test_new_users_are_folded_in_and_ranked():
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.ranking import restate_scores

    n_users, n_items, K = 12, 10, 3
    rng = np.random.RandomState(4)
    taste, look = rng.randn(n_users + 4, 3), rng.randn(n_items, 3)

    def rows(users, per_user, width):
        u = np.repeat(users, per_user)
        it = np.concatenate([rng.choice(n_items, per_user, replace=False) for _ in users])
        uc = np.where(u < n_users, u, u + n_items)  # new users come after the items
        X = sp.csr_matrix((np.ones(2 * u.size), np.stack([uc, n_users + it], 1).ravel(),
                           2 * np.arange(u.size + 1)), shape=(u.size, width))
        X.sort_indices()
        return X, (taste[u] * look[it]).sum(axis=1) + 0.5 * taste[u, 0]

    d = n_users + n_items
    X, y = rows(np.arange(n_users), 7, d)
    est = SparseFactorizationMachineRegressor(degree=2, n_components=4, alpha=0.05, beta=0.05,
                                              gamma=1e-4, max_iter=30, tol=1e-4, random_state=0,
                                              precision="f64", device=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, y)
    new = est.extend_features(4)
    assert new.tolist() == [d, d + 1, d + 2, d + 3] and est.P_.shape[2] == d + 4
    Xn, yn = rows(n_users + np.arange(4), 6, d + 4)
    before = 0.5 * ((est.predict(Xn) - yn) ** 2).sum()
    res = est.fold_in(Xn, yn, new, update=True)
    after = 0.5 * ((est.predict(Xn) - yn) ** 2).sum()
    assert res.converged.all() and (res.n_rows == 6).all() and (res.n_iter <= 2).all()
    assert (res.objective_after < res.objective_before).all()
    np.testing.assert_allclose(res.objective_before.sum(), before, rtol=1e-9)
    assert after < before
    print("loss over the new users' rows: %.4g -> %.4g" % (before, after))
    ctx = sp.csr_matrix((np.ones(4), new, np.arange(5)), shape=(4, d + 4))
    cand = sp.csr_matrix((np.ones(n_items), n_users + np.arange(n_items), np.arange(n_items + 1)),
                         shape=(n_items, d + 4))
    S = restate_scores(est, ctx, cand)
    top = -np.sort(-S, axis=1)[:, :K + 1]
    assert np.diff(-top, axis=1).min() > CLEAR * np.abs(S).max(), "top K + 1 scores too close"
    with est.ranker(cand) as r:
        idx, val = r.top_k(ctx, K)
    assert (idx == np.argsort(-S, axis=1, kind="stable")[:, :K]).all()
    # the new users' scores differ: their columns are in use
    assert len({tuple(row) for row in np.round(S, 6)}) == 4


# ---------------------------------------------------------------- 4. refusals, raw C entry
def _raw_call(eng, pr, X, y, cols, beta=BETA, R=None):
    """-> (return code, outputs) with the outputs pre-filled with sentinels"""
    from sparsepoly_amd import _capi

    Xr, args, keep = eng._explain_args(X, pr.blocks, pr.coef, pr.lin, "foldin")
    ya, yp = _capi.f64(y)
    ca, cp = _capi.i32(cols)
    m, R = len(ca), (pr.R if R is None else R)
    out = dict(theta=np.full((m, R), 7.0), n_rows=np.full(m, -7, dtype=np.int64),
               n_iter=np.full(m, -7, dtype=np.int32), conv=np.full(m, -7, dtype=np.int32),
               gn=np.full(m, 7.0), o0=np.full(m, 7.0), o1=np.full(m, 7.0))
    ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))  # noqa: E731
    rc = eng._lib.spfm_foldin_csr(
        *args[:5], yp, *args[5:], float(pr.offset), _capi.LOSSES[pr.loss], m, cp, ALPHA, beta, 50,
        TOL, ptr(out["theta"], ctypes.c_double), ptr(out["n_rows"], ctypes.c_int64),
        ptr(out["n_iter"], ctypes.c_int32), ptr(out["conv"], ctypes.c_int32),
        ptr(out["gn"], ctypes.c_double), ptr(out["o0"], ctypes.c_double),
        ptr(out["o1"], ctypes.c_double))
    return rc, out


def _untouched(out):
    return all((np.abs(v) == 7).all() for v in out.values())


def test_refusals_leave_the_outputs_alone():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.foldin import _problem

    d = 40
    targets = np.array([5, 9])
    X = target_rows(d, targets, [3, 4], [1, 2, 6], n_ignored=2)
    est = estimator(2, "explicit", True, 6, "squared", d=d)
    y = targets_for(est, X.shape[0])
    pr = _problem(est, X, y, targets, None, None, 50, TOL)
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(pr.P, pr.w, pr.lams)
        rc, out = _raw_call(eng, pr, X, y, targets)
        assert rc == _capi.SPFM_OK and not _untouched(out) and out["n_rows"].tolist() == [3, 4]
        good = out
        two = sp.vstack([X, sp.csr_matrix(([1.0, 2.0], ([0, 0], [5, 9])), shape=(1, d))]).tocsr()
        for what, code, a in (
                ("two targets in row %d" % X.shape[0], _capi.SPFM_ERR_INVALID,
                 (two, np.append(y, 0.0), targets)),
                ("duplicate column", _capi.SPFM_ERR_INVALID, (X, y, [5, 5])),
                ("column out of range", _capi.SPFM_ERR_INVALID, (X, y, [5, d])),
                ("beta = 0", _capi.SPFM_ERR_INVALID, (X, y, targets, 0.0))):
            rc, out = _raw_call(eng, pr, *a)
            assert rc == code and _untouched(out), what
            msg = eng._lib.spfm_last_error(eng._h).decode()
            if what.startswith("two"):
                assert "row %d " % X.shape[0] in msg, msg
        # n = 0 is valid: only the zero-row results are written
        rc, out = _raw_call(eng, pr, sp.csr_matrix((0, d)), np.zeros(0), targets)
        assert rc == _capi.SPFM_OK
        assert (out["theta"] == 0).all() and (out["n_rows"] == 0).all()
        assert (out["n_iter"] == 0).all() and (out["conv"] == 1).all()
        assert (out["gn"] == 0).all() and (out["o0"] == 0).all() and (out["o1"] == 0).all()
        assert eng.foldin_info()["groups"] == 0
        # the handle still answers, bit for bit
        rc, out = _raw_call(eng, pr, X, y, targets)
        assert rc == _capi.SPFM_OK and all((out[n] == good[n]).all() for n in out)
    finally:
        eng.close()
    # R = 129: two blocks of 64 components and a linear term
    big = estimator(3, "explicit", True, 64, "squared", d=d)
    pb = _problem(estimator(3, "explicit", False, 64, "squared", d=d), X, y, targets, None, None,
                  50, TOL)
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(big.P_, big.w_, big.lams_)
        pb.lin = True
        rc, out = _raw_call(eng, pb, X, y, targets, R=129)
        assert rc == _capi.SPFM_ERR_UNSUPPORTED and _untouched(out)
        assert "SPFM_FOLDIN_MAX_UNKNOWNS" in eng._lib.spfm_last_error(eng._h).decode()
    finally:
        eng.close()
