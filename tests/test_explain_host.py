"""``sparsepoly_amd.explain`` without a device: the NumPy restatement ``restate_contributions``
against brute-force Shapley values (every subset of a row's stored entries, the others zeroed,
through ``ranking._restate_output``), the efficiency identity, the gradient against central
differences, the four new symbols and the argument errors that are raised before any device use.
``rows_matrix``, ``model_output`` and ``majorant`` are shared with ``tests/test_hip_explain.py``."""
import itertools
import os
import re
from math import factorial

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from sklearn.utils.validation import NotFittedError
from test_ranking_host import abs_model, all_subsets, fm

COMBOS = list(itertools.product((2, 3, 4, 5, 6), ("explicit", "augment", None), (True, False)))


def rows_matrix(lengths, d, seed=0, f32=False):
    """CSR (len(lengths), d): row i stores lengths[i] standard-normal entries at random columns"""
    rng = np.random.RandomState(seed + 2000)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(d, size=m, replace=False)) for m in lengths]
                         + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = rng.randn(int(indptr[-1]))
    if f32:
        data = data.astype(np.float32).astype(np.float64)
    return sp.csr_matrix((data, idx, indptr), shape=(len(lengths), d))


def model_output(est, V, dtype=np.double):
    """what ``_get_output`` computes on the dense rows V (n, n_features), dummy columns added"""
    from sparsepoly_amd.ranking import _restate_output, _spec

    degree, lin, lower, P, w, lams = _spec(est)
    Va = np.asarray(sp.csr_matrix(est._augment(sp.csr_matrix(np.asarray(V, dtype=np.double))))
                    .todense())
    return _restate_output(Va, degree, lin, lower, P, w, lams, dtype)


def majorant(est, X, mode):
    """S_hat per stored entry of the canonical X, in longdouble: the sum of the magnitudes of the
    terms a computed value is made of,
        |w_j x_ij| + sum_s |p x| sum_t (|c_st| / t) sum_r |p x|^r A^{t-1-r}(|p_s|, |x_i|)
    (gradient: without the leading |x_ij| and the 1 / t).  The inner sum over r is the downdate
    with every sign +: G_0 = 1, G_t = a_t + |p x| G_{t-1}.  |c_st| is taken from the model of
    magnitudes, which also majorises the terms the host's coefficients are made of."""
    from sparsepoly_amd.explain import _model

    ld = np.longdouble
    Xc, blocks, coef, P, w, lams, lin, base = _model(abs_model(est), X, ld)
    P, w = P.astype(ld), w.astype(ld)
    V = np.abs(np.asarray(Xc.todense(), dtype=ld))
    out = np.zeros(V.shape, dtype=ld)
    used = np.flatnonzero((V != 0).any(axis=0))
    for q, (o, m) in enumerate(blocks):
        for s0 in range(0, P.shape[1], 16):
            Ps, c = P[o, s0:s0 + 16], coef[q, s0:s0 + 16]
            PX = Ps[None] * V[:, None, :]
            a = [np.ones(PX.shape[:2], dtype=ld)] + [np.zeros(PX.shape[:2], dtype=ld)
                                                     for _ in range(m)]
            for j in used:
                for t in range(m, 0, -1):
                    a[t] = a[t] + a[t - 1] * PX[:, :, j]
            G = np.ones(PX.shape, dtype=ld)
            inner = np.zeros(PX.shape, dtype=ld)
            for t in range(1, m + 1):
                if t > 1:
                    G = a[t - 1][:, :, None] + PX * G
                ct = c[:, t] / t if mode == "attribution" else c[:, t]
                inner = inner + ct[None, :, None] * G
            out += (Ps[None] * inner).sum(axis=1)
    if lin:
        out += w[None, :]
    if mode == "attribution":
        out *= V
    rows = np.repeat(np.arange(V.shape[0]), np.diff(Xc.indptr))
    return out[rows, Xc.indices], base


def brute_force_shapley(est, x):
    """Shapley values of the stored entries of the dense row x against the baseline 0, from the
    model's output on all 2^n rows that keep a subset of them"""
    cols = np.flatnonzero(x)
    n = len(cols)
    masks = list(itertools.product((0, 1), repeat=n))
    V = np.zeros((len(masks), x.shape[0]))
    for r, mk in enumerate(masks):
        V[r, cols] = x[cols] * np.array(mk)
    f = dict(zip(masks, model_output(est, V)))
    phi = np.zeros(n)
    for q in range(n):
        for mk in masks:
            if mk[q]:
                continue
            r = sum(mk)
            with_q = mk[:q] + (1,) + mk[q + 1:]
            phi[q] += factorial(r) * factorial(n - r - 1) / factorial(n) * (f[with_q] - f[mk])
    return cols, phi, f[(0,) * n]


def _cases():
    from sparsepoly_amd import SparseFactorizationMachineClassifier

    cases = [pytest.param((None, dg, fl, lin), id="reg-%d-%s-%d" % (dg, fl, lin))
             for dg, fl, lin in COMBOS]
    cases.append(pytest.param((SparseFactorizationMachineClassifier, 3, "explicit", True),
                              id="classifier-3-explicit-1"))
    cases.append(pytest.param((SparseFactorizationMachineClassifier, 4, "augment", True),
                              id="classifier-4-augment-1"))
    return cases


@pytest.mark.parametrize("spec", _cases())
def test_restatement_equals_brute_force_shapley(spec):
    """rows of 0, 1, 3 and 6 stored entries; agreement to 1e-12 of the sum of magnitudes: per row
    the output of the model of magnitudes on |x| (the brute-force side's terms) plus the
    majorants of its entries (the formula's terms: the downdate adds terms that cancel, so a
    degree-4 block on a 3-entry row restates an exact 0 as 1e-17).  The rows sum to the output
    minus the base value, and the base value is the output on an empty row"""
    from sparsepoly_amd.explain import restate_contributions

    cls, degree, fl, lin = spec
    est = fm(degree, 3, 9, fl, lin, seed=10 + degree, cls=cls)
    X = rows_matrix([0, 1, 3, 6], 9, seed=degree)
    Xc, vals, base = restate_contributions(est, X, "attribution")
    assert (Xc.indptr == X.indptr).all() and (Xc.indices == X.indices).all()
    Xd = X.toarray()
    f = model_output(est, Xd)
    S_abs = model_output(abs_model(est), np.abs(Xd))
    S_hat = majorant(est, X, "attribution")[0].astype(np.double)
    assert np.abs(vals).max() > 0  # (degree 6 on 6 entries: one monomial of six small factors)
    for i in range(X.shape[0]):
        cols, phi, f0 = brute_force_shapley(est, Xd[i])
        got = vals[X.indptr[i]:X.indptr[i + 1]]
        assert (cols == X.indices[X.indptr[i]:X.indptr[i + 1]]).all()
        tol = 1e-12 * (S_abs[i] + S_hat[X.indptr[i]:X.indptr[i + 1]].sum())
        assert np.abs(got - phi).max(initial=0.0) <= tol
        assert abs(f0 - base) <= tol
        assert abs(got.sum() + base - f[i]) <= tol


@pytest.mark.parametrize("degree,fl,lin", COMBOS)
def test_gradient_equals_central_differences(degree, fl, lin):
    """A property of the formula, not a device tolerance: in longdouble, step 1e-6, the largest
    difference is below 1e-6 of the largest gradient (the differences' own error is
    h^2 f''' / 6, about 1e-12 of the third derivative)."""
    from sparsepoly_amd.explain import restate_contributions

    est = fm(degree, 3, 9, fl, lin, seed=20 + degree)
    X = rows_matrix([0, 1, 3, 6], 9, seed=degree)
    Xc, grad, _ = restate_contributions(est, X, "gradient", wide=True)
    assert grad.dtype == np.longdouble
    Xd = X.toarray().astype(np.longdouble)
    h = np.longdouble(1e-6)
    fd = np.zeros(X.nnz, dtype=np.longdouble)
    for i in range(X.shape[0]):
        for e in range(X.indptr[i], X.indptr[i + 1]):
            hi, lo = Xd[i].copy(), Xd[i].copy()
            hi[X.indices[e]] += h
            lo[X.indices[e]] -= h
            fpm = _wide_output(est, np.stack([hi, lo]))
            fd[e] = (fpm[0] - fpm[1]) / (2 * h)
    assert np.abs(grad).max() > 0
    assert np.abs(fd - grad).max() <= 1e-6 * np.abs(grad).max()


def _wide_output(est, V):
    """``model_output`` in longdouble on longdouble rows (the dummy columns by hand: scipy keeps
    no longdouble)"""
    from sparsepoly_amd.explain import _columns
    from sparsepoly_amd.ranking import _restate_output, _spec

    degree, lin, lower, P, w, lams = _spec(est)
    real, dummy = _columns(est, V.shape[1])
    Va = np.zeros((V.shape[0], real.size + dummy.size), dtype=np.longdouble)
    Va[:, real] = V
    Va[:, dummy] = 1
    return _restate_output(Va, degree, lin, lower, P, w, lams, np.longdouble)


def test_wide_restatement_agrees_with_the_double_one():
    from sparsepoly_amd.explain import restate_contributions

    est = fm(4, 3, 9, "augment", True)
    X = rows_matrix([0, 2, 5], 9)
    for mode in ("attribution", "gradient"):
        _, v, b = restate_contributions(est, X, mode)
        _, vw, bw = restate_contributions(est, X, mode, wide=True)
        assert v.dtype == np.double and vw.dtype == np.longdouble
        np.testing.assert_allclose(v, vw.astype(np.double), rtol=0, atol=1e-13)
        assert abs(b - float(bw)) < 1e-13


def test_majorant_dominates_the_values():
    """|phi| <= S_hat entry by entry (the triangle inequality the device bound rests on)"""
    from sparsepoly_amd.explain import restate_contributions

    for degree, fl in ((3, "explicit"), (5, "augment"), (6, None)):
        est = fm(degree, 4, 12, fl, True, seed=degree)
        X = rows_matrix([0, 3, 7, 12], 12, seed=degree)
        for mode in ("attribution", "gradient"):
            _, v, _ = restate_contributions(est, X, mode, wide=True)
            S, _ = majorant(est, X, mode)
            assert (np.abs(v) <= S * (1 + 1e-15)).all()


def test_header_capi_and_library_agree_on_the_new_symbols():
    from sparsepoly_amd import _capi

    names = ("spfm_explain_csr", "spfm_explain_topk_csr", "spfm_explain_set_partition",
             "spfm_explain_info")
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS
    assert re.search(r"#define SPFM_EXPLAIN_MAX_K %d\b" % _capi.EXPLAIN_MAX_K, header)
    for mode, value in _capi.EXPLAIN_MODES.items():
        assert re.search(r"#define SPFM_EXPLAIN_%s %d\b" % (mode.upper(), value), header)
    lib = _capi.load()
    for name in names:
        assert hasattr(lib, name), name


def test_argument_errors_come_before_any_device_use(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRegressor, engine
    from sparsepoly_amd.explain import restate_contributions

    def no_device(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", no_device)
    X = rows_matrix([0, 2, 3], 10)
    for est in (fm(2, 3, 10), fm(4, 3, 10, "augment")):
        for call in (lambda: est.feature_contributions(X[:, :9]),
                     lambda: est.input_gradient(sp.csr_matrix((2, 12))),
                     lambda: est.top_contributions(X[:, :9], 3),
                     lambda: restate_contributions(est, X[:, :9], "attribution")):
            with pytest.raises(ValueError, match="features"):
                call()
        for K in (0, -1, 2.5):
            with pytest.raises(ValueError, match="K must be"):
                est.top_contributions(X, K)
        with pytest.raises(ValueError, match="exceeds the cap"):
            est.top_contributions(X, 65)
        with pytest.raises(ValueError, match="mode must be"):
            restate_contributions(est, X, "shap")
    unfitted = SparseFactorizationMachineRegressor()
    for call in (lambda: unfitted.feature_contributions(X), lambda: unfitted.input_gradient(X),
                 lambda: unfitted.top_contributions(X, 1),
                 lambda: restate_contributions(unfitted, X, "gradient")):
        with pytest.raises(NotFittedError):
            call()
    # reaching the device is the only thing left to go wrong for good arguments
    with pytest.raises(AssertionError, match="device handle"):
        fm(2, 3, 10).feature_contributions(X)


def test_all_subsets_estimators_do_not_explain():
    est = all_subsets(3, 8)
    for name in ("feature_contributions", "input_gradient", "top_contributions"):
        assert not hasattr(est, name)


def test_inputs_are_canonicalised_and_left_alone():
    """unsorted indices and duplicates: summed, the pattern is the canonical one and the
    caller's arrays are not changed; CSC and dense input give the same values"""
    from sparsepoly_amd.explain import restate_contributions

    est = fm(3, 2, 8)
    X = rows_matrix([0, 3, 5], 8)
    Xc = X.tocoo()
    rows = np.concatenate([Xc.row, Xc.row])[::-1]
    cols = np.concatenate([Xc.col, Xc.col])[::-1]
    vals = np.concatenate([0.25 * Xc.data, 0.75 * Xc.data])[::-1]
    Xdup = sp.coo_matrix((vals, (rows, cols)), shape=X.shape).tocsc()
    before = Xdup.data.copy()
    want = restate_contributions(est, X, "attribution")
    for form in (Xdup, X.tocsc(), X.toarray()):
        got = restate_contributions(est, form, "attribution")
        assert (got[0].indptr == X.indptr).all() and (got[0].indices == X.indices).all()
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-13)
    assert (Xdup.data == before).all()
