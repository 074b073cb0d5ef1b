"""The pair attributions of ``sparsepoly_amd.explain`` without a device: the NumPy restatement
``restate_pair_contributions`` against brute-force Shapley-Taylor indices of order 2 (every subset
of a row's stored entries, the others zeroed), the three identities (efficiency, consistency with
``restate_contributions``, ``x_a x_b W[a, b]`` for a plain degree-2 model), the hessian against
central second differences, the new symbols and the argument errors that are raised before any
device use.  ``pair_majorant`` and ``numpy_groups`` are shared with ``tests/test_hip_pairs.py``."""
import itertools
import os
import re
from math import comb

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from sklearn.utils.validation import NotFittedError
from test_explain_host import COMBOS, _wide_output, majorant, model_output, rows_matrix
from test_ranking_host import abs_model, all_subsets, fm

PAIR_METHODS = ("pair_contributions", "top_pair_contributions", "group_contributions")


def pair_majorant(est, X, mode):
    """``(S_pairs, S_main, base_abs)`` in longdouble: per pair and per stored entry of the
    canonical X the sum of the magnitudes of the terms a computed value is made of,
        sum_s |z_a| |z_b| sum_t |c_st| 2 / (t (t - 1)) H_{t-2},   |w_a x_a| + sum_s |c_s1| |z_a|
    (hessian: |p_a| |p_b| in front and no 2 / (t (t - 1))), with both downdates taken with every
    sign +: G_t = a_t + |z_a| G_{t-1}, H_t = G_t + |z_b| H_{t-1} on the model of magnitudes, which
    also majorises the terms the host's coefficients are made of."""
    from sparsepoly_amd.explain import _model, pair_columns

    ld = np.longdouble
    Xc, blocks, coef, P, w, lams, lin, base = _model(abs_model(est), X, ld)
    P, w = P.astype(ld), w.astype(ld)
    ptr, _, _ = pair_columns(Xc)
    S = np.zeros(int(ptr[-1]), dtype=ld)
    Sm = np.zeros(Xc.nnz, dtype=ld)
    for i in range(Xc.shape[0]):
        lo, hi = Xc.indptr[i], Xc.indptr[i + 1]
        cols, x = Xc.indices[lo:hi], np.abs(Xc.data[lo:hi].astype(ld))
        m = hi - lo
        if m == 0:
            continue
        ia, ib = np.triu_indices(m, 1)
        if lin:
            Sm[lo:hi] += w[cols] * x
        for q, (o, M) in enumerate(blocks):
            for s0 in range(0, P.shape[1], 16):
                Pc, c = P[o][s0:s0 + 16][:, cols], coef[q][s0:s0 + 16]
                Z = Pc * x[None, :]
                a = [np.ones(Z.shape[0], dtype=ld)] + [np.zeros(Z.shape[0], dtype=ld)
                                                       for _ in range(M)]
                for j in range(m):
                    for t in range(M, 0, -1):
                        a[t] = a[t] + a[t - 1] * Z[:, j]
                Sm[lo:hi] += (c[:, 1][:, None] * Z).sum(axis=0)
                if m < 2:
                    continue
                za, zb = Z[:, ia], Z[:, ib]
                G = np.ones(za.shape, dtype=ld)
                H = np.ones(za.shape, dtype=ld)
                inner = np.zeros(za.shape, dtype=ld)
                for t in range(2, M + 1):
                    if t > 2:
                        G = a[t - 2][:, None] + za * G
                        H = G + zb * H
                    ct = c[:, t] * 2 / (t * (t - 1)) if mode == "interaction" else c[:, t]
                    inner = inner + ct[:, None] * H
                lead = za * zb if mode == "interaction" else Pc[:, ia] * Pc[:, ib]
                S[ptr[i]:ptr[i + 1]] += (lead * inner).sum(axis=0)
    return S, Sm, base


def numpy_groups(Xc, ptr, vals, main, groups, G):
    """(T (n, G, G) upper-triangular, main per group (n, G)) of flat pair values, in their dtype"""
    n = Xc.shape[0]
    T = np.zeros((n, G, G), dtype=vals.dtype)
    mg = np.zeros((n, G), dtype=main.dtype)
    for i in range(n):
        lo, hi = Xc.indptr[i], Xc.indptr[i + 1]
        g = np.asarray(groups)[Xc.indices[lo:hi]]
        np.add.at(mg[i], g, main[lo:hi])
        if hi - lo > 1:
            ia, ib = np.triu_indices(hi - lo, 1)
            np.add.at(T[i], (np.minimum(g[ia], g[ib]), np.maximum(g[ia], g[ib])),
                      vals[ptr[i]:ptr[i + 1]])
    return T, mg


def brute_force_shapley_taylor(est, x):
    """Shapley-Taylor indices of order 2 of the stored entries of the dense row x against the
    baseline 0, from the model's output on all 2^n rows that keep a subset of them:
        I_a  = f({a}) - f({}),
        I_ab = (2 / n) sum over T in N - {a, b} of
               (f(T + a + b) - f(T + a) - f(T + b) + f(T)) / C(n - 1, |T|)
    -> (cols, main (n), pairs (n (n - 1) / 2, first then second member), f({}))"""
    cols = np.flatnonzero(x)
    n = len(cols)
    masks = list(itertools.product((0, 1), repeat=n))
    V = np.zeros((len(masks), x.shape[0]))
    for r, mk in enumerate(masks):
        V[r, cols] = x[cols] * np.array(mk)
    f = dict(zip(masks, model_output(est, V)))
    empty = (0,) * n

    def put(mk, *on):
        mk = list(mk)
        for q in on:
            mk[q] = 1
        return tuple(mk)

    main = np.array([f[put(empty, a)] - f[empty] for a in range(n)])
    pairs = []
    for a, b in itertools.combinations(range(n), 2):
        tot = 0.0
        for mk in masks:
            if mk[a] or mk[b]:
                continue
            delta = f[put(mk, a, b)] - f[put(mk, a)] - f[put(mk, b)] + f[mk]
            tot += delta / comb(n - 1, sum(mk))
        pairs.append(2.0 / n * tot)
    return cols, main, np.array(pairs), f[empty]


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
def test_restatement_equals_brute_force_shapley_taylor(spec):
    """rows of 0, 1, 2, 3 and 6 stored entries; agreement to 1e-12 of the sum of magnitudes: per
    row the output of the model of magnitudes on |x| (the brute-force side's terms) plus the
    majorants of its pairs and entries (the formula's terms, the cancelling downdate terms
    counted by magnitude).  Identity (1): the row's values sum to the output minus the base."""
    from sparsepoly_amd.explain import restate_pair_contributions

    cls, degree, fl, lin = spec
    est = fm(degree, 3, 9, fl, lin, seed=10 + degree, cls=cls)
    X = rows_matrix([0, 1, 2, 3, 6], 9, seed=degree)
    Xc, ptr, ca, cb, vals, main, base = restate_pair_contributions(est, X, "interaction")
    assert (Xc.indptr == X.indptr).all() and (Xc.indices == X.indices).all()
    assert list(np.diff(ptr)) == [0, 0, 1, 3, 15] and (ca < cb).all()
    Xd = X.toarray()
    f = model_output(est, Xd)
    S_abs = model_output(abs_model(est), np.abs(Xd))
    S, Sm, _ = pair_majorant(est, X, "interaction")
    assert np.abs(vals).max() > 0
    for i in range(X.shape[0]):
        cols, bmain, bpairs, f0 = brute_force_shapley_taylor(est, Xd[i])
        lo, hi = X.indptr[i], X.indptr[i + 1]
        assert (cols == X.indices[lo:hi]).all()
        ia, ib = np.triu_indices(hi - lo, 1)
        assert (ca[ptr[i]:ptr[i + 1]] == cols[ia]).all()
        assert (cb[ptr[i]:ptr[i + 1]] == cols[ib]).all()
        tol = 1e-12 * float(S_abs[i] + S[ptr[i]:ptr[i + 1]].sum() + Sm[lo:hi].sum())
        assert np.abs(vals[ptr[i]:ptr[i + 1]] - bpairs).max(initial=0.0) <= tol
        assert np.abs(main[lo:hi] - bmain).max(initial=0.0) <= tol
        assert abs(f0 - base) <= tol
        assert abs(main[lo:hi].sum() + vals[ptr[i]:ptr[i + 1]].sum() + base - f[i]) <= tol


@pytest.mark.parametrize("degree,fl,lin", COMBOS)
def test_pairs_and_main_add_up_to_the_feature_contributions(degree, fl, lin):
    """identity (2): phi_ia = main_ia + 1/2 sum_{b != a} phi_iab, against
    ``restate_contributions``, to 1e-12 of the two majorants"""
    from sparsepoly_amd.explain import restate_contributions, restate_pair_contributions

    est = fm(degree, 4, 12, fl, lin, seed=20 + degree)
    X = rows_matrix([0, 1, 2, 5, 12], 12, seed=degree)
    Xc, want, base = restate_contributions(est, X, "attribution", wide=True)
    _, ptr, ca, cb, vals, main, base2 = restate_pair_contributions(est, X, "interaction", wide=True)
    assert vals.dtype == np.longdouble and main.dtype == np.longdouble
    assert base == base2
    S, Sm, _ = pair_majorant(est, X, "interaction")
    S1, _ = majorant(est, X, "attribution")
    got, tol = main.copy(), Sm + S1
    for i in range(Xc.shape[0]):
        lo, hi = Xc.indptr[i], Xc.indptr[i + 1]
        if hi - lo > 1:
            ia, ib = np.triu_indices(hi - lo, 1)
            for side in (ia, ib):
                np.add.at(got, lo + side, vals[ptr[i]:ptr[i + 1]] / 2)
                np.add.at(tol, lo + side, S[ptr[i]:ptr[i + 1]])
    assert np.abs(want).max() > 0
    assert (np.abs(got - want) <= 1e-12 * tol).all()


@pytest.mark.parametrize("fl", ["explicit", "augment", None])
def test_a_plain_degree_2_model_gives_x_x_w(fl):
    """identity (3): phi_iab = x_ia x_ib W[a, b], W = sum_s lams_s p_s p_s^T on the real columns;
    with 'augment' and a linear term degree 2 has no dummy column either"""
    from sparsepoly_amd.explain import restate_pair_contributions

    est = fm(2, 5, 12, fl, True, seed=3)
    X = rows_matrix([0, 1, 2, 7, 12], 12, seed=3)
    Xc, ptr, ca, cb, vals, main, base = restate_pair_contributions(est, X, "interaction")
    P = est.P_[0][:, :12]
    W = P.T @ (est.lams_[:, None] * P)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(ptr))
    Xd = X.toarray()
    want = Xd[rows, ca] * Xd[rows, cb] * W[ca, cb]
    np.testing.assert_allclose(vals, want, rtol=0, atol=1e-13 * np.abs(want).max())
    np.testing.assert_allclose(main, est.w_[Xc.indices] * Xc.data, rtol=0, atol=1e-14)
    _, _, _, _, hess, hmain, _ = restate_pair_contributions(est, X, "hessian")
    np.testing.assert_allclose(hess, W[ca, cb], rtol=0, atol=1e-13 * np.abs(W).max())
    assert (hmain == 0).all()


@pytest.mark.parametrize("degree,fl,lin", COMBOS)
def test_hessian_equals_central_second_differences(degree, fl, lin):
    """A property of the formula, not a device tolerance: in longdouble, step 1e-4, the largest
    difference is below 1e-6 of the largest value (the differences' own error is h^2 / 6 times a
    fourth derivative, about 1e-9, their rounding 1e-19 / h^2 = 1e-11)."""
    from sparsepoly_amd.explain import restate_pair_contributions

    est = fm(degree, 3, 9, fl, lin, seed=20 + degree)
    X = rows_matrix([0, 1, 2, 3, 6], 9, seed=degree)
    Xc, ptr, ca, cb, hess, _, _ = restate_pair_contributions(est, X, "hessian", wide=True)
    assert hess.dtype == np.longdouble
    Xd = X.toarray().astype(np.longdouble)
    h = np.longdouble(1e-4)
    fd = np.zeros(hess.shape, dtype=np.longdouble)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(ptr))
    for q in range(hess.shape[0]):
        pts = []
        for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            v = Xd[rows[q]].copy()
            v[ca[q]] += sa * h
            v[cb[q]] += sb * h
            pts.append(v)
        fpm = _wide_output(est, np.stack(pts))
        fd[q] = (fpm[0] - fpm[1] - fpm[2] + fpm[3]) / (4 * h * h)
    assert np.abs(hess).max() > 0
    assert np.abs(fd - hess).max() <= 1e-6 * np.abs(hess).max()


def test_wide_restatement_agrees_with_the_double_one():
    from sparsepoly_amd.explain import restate_pair_contributions

    est = fm(4, 3, 9, "augment", True)
    X = rows_matrix([0, 2, 5], 9)
    for mode in ("interaction", "hessian"):
        r = restate_pair_contributions(est, X, mode)
        rw = restate_pair_contributions(est, X, mode, wide=True)
        assert r[4].dtype == np.double and rw[4].dtype == np.longdouble
        np.testing.assert_allclose(r[4], rw[4].astype(np.double), rtol=0, atol=1e-13)
        np.testing.assert_allclose(r[5], rw[5].astype(np.double), rtol=0, atol=1e-13)
        assert abs(r[6] - float(rw[6])) < 1e-13


def test_majorant_dominates_the_values():
    """|phi| <= S_hat pair by pair and entry by entry (the triangle inequality the device bound
    rests on)"""
    from sparsepoly_amd.explain import restate_pair_contributions

    for degree, fl in ((3, "explicit"), (5, "augment"), (6, None)):
        est = fm(degree, 4, 12, fl, True, seed=degree)
        X = rows_matrix([0, 3, 7, 12], 12, seed=degree)
        for mode in ("interaction", "hessian"):
            r = restate_pair_contributions(est, X, mode, wide=True)
            S, Sm, _ = pair_majorant(est, X, mode)
            assert (np.abs(r[4]) <= S * (1 + 1e-15)).all()
            if mode == "interaction":
                assert (np.abs(r[5]) <= Sm * (1 + 1e-15)).all()


def test_group_tables_add_up():
    """the NumPy grouping of the restatement: upper-triangular, every pair in exactly one cell"""
    from sparsepoly_amd.explain import restate_pair_contributions

    est = fm(3, 4, 12, "explicit", True, seed=4)
    X = rows_matrix([0, 1, 5, 12], 12, seed=4)
    Xc, ptr, ca, cb, vals, main, base = restate_pair_contributions(est, X, "interaction")
    groups = np.arange(12) % 3
    T, mg = numpy_groups(Xc, ptr, vals, main, groups, 3)
    assert (np.tril(T, -1) == 0).all()
    f = model_output(est, X.toarray())
    np.testing.assert_allclose(T.sum((1, 2)) + mg.sum(1) + base, f, rtol=0, atol=1e-12)


def test_header_capi_and_library_agree_on_the_new_symbols():
    from sparsepoly_amd import _capi

    names = ("spfm_explain_pairs_csr", "spfm_explain_pairs_topk_csr",
             "spfm_explain_pairs_grouped_csr")
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS
    assert re.search(r"#define SPFM_PAIRS_MAX_K %d\b" % _capi.PAIRS_MAX_K, header)
    assert re.search(r"#define SPFM_PAIRS_MAX_GROUPS %d\b" % _capi.PAIRS_MAX_GROUPS, header)
    assert re.search(r"#define SPFM_PAIRS_MAX_BYTES \(1ll << 30\)", header)
    assert _capi.PAIRS_MAX_BYTES == 1 << 30
    for mode, value in _capi.PAIRS_MODES.items():
        assert re.search(r"#define SPFM_PAIRS_%s %d\b" % (mode.upper(), value), header)
    lib = _capi.load()
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) >= 13, name


def test_argument_errors_come_before_any_device_use(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRegressor, engine
    from sparsepoly_amd.explain import restate_pair_contributions

    def no_device(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", no_device)
    X = rows_matrix([0, 2, 3], 10)
    groups = np.arange(10) % 2
    for est in (fm(2, 3, 10), fm(4, 3, 10, "augment")):
        for call in (lambda: est.pair_contributions(X[:, :9]),
                     lambda: est.top_pair_contributions(sp.csr_matrix((2, 12)), 3),
                     lambda: est.group_contributions(X[:, :9], groups[:9]),
                     lambda: restate_pair_contributions(est, X[:, :9], "interaction")):
            with pytest.raises(ValueError, match="features"):
                call()
        for K in (0, -1, 2.5):
            with pytest.raises(ValueError, match="K must be"):
                est.top_pair_contributions(X, K)
        with pytest.raises(ValueError, match="exceeds the cap"):
            est.top_pair_contributions(X, 65)
        for call in (lambda: est.pair_contributions(X, mode="shap"),
                     lambda: est.top_pair_contributions(X, 2, mode="attribution"),
                     lambda: restate_pair_contributions(est, X, "gradient")):
            with pytest.raises(ValueError, match="mode must be"):
                call()
        with pytest.raises(ValueError, match="return_main"):
            est.pair_contributions(X, mode="hessian", return_main=True)
        with pytest.raises(ValueError, match="one id per feature"):
            est.group_contributions(X, groups[:9])
        with pytest.raises(ValueError, match="integer array"):
            est.group_contributions(X, groups.astype(float))
        with pytest.raises(ValueError, match="ids >= 0"):
            est.group_contributions(X, groups - 1)
        with pytest.raises(ValueError, match="more than the cap"):
            est.group_contributions(X, np.arange(10) * 4)
    unfitted = SparseFactorizationMachineRegressor()
    for call in (lambda: unfitted.pair_contributions(X),
                 lambda: unfitted.top_pair_contributions(X, 1),
                 lambda: unfitted.group_contributions(X, groups),
                 lambda: restate_pair_contributions(unfitted, X, "hessian")):
        with pytest.raises(NotFittedError):
            call()
    # reaching the device is the only thing left to go wrong for good arguments
    for call in (lambda: fm(2, 3, 10).pair_contributions(X),
                 lambda: fm(2, 3, 10).top_pair_contributions(X, 64),
                 lambda: fm(2, 3, 10).group_contributions(X, groups)):
        with pytest.raises(AssertionError, match="device handle"):
            call()


def test_all_subsets_estimators_have_none_of_the_methods():
    est = all_subsets(3, 8)
    for name in PAIR_METHODS:
        assert not hasattr(est, name)
    for name in PAIR_METHODS:
        assert hasattr(fm(2, 3, 8), name)


def test_inputs_are_canonicalised_and_left_alone():
    """unsorted indices and duplicates: summed, the pairs are those of the canonical pattern and
    the caller's arrays are not changed; CSC and dense input give the same values"""
    from sparsepoly_amd.explain import restate_pair_contributions

    est = fm(3, 2, 8)
    X = rows_matrix([0, 3, 5], 8)
    Xc = X.tocoo()
    rows = np.concatenate([Xc.row, Xc.row])[::-1]
    cols = np.concatenate([Xc.col, Xc.col])[::-1]
    vals = np.concatenate([0.25 * Xc.data, 0.75 * Xc.data])[::-1]
    Xdup = sp.coo_matrix((vals, (rows, cols)), shape=X.shape).tocsc()
    before = Xdup.data.copy()
    want = restate_pair_contributions(est, X, "interaction")
    assert list(np.diff(want[1])) == [0, 3, 10]
    for form in (Xdup, X.tocsc(), X.toarray()):
        got = restate_pair_contributions(est, form, "interaction")
        assert (got[0].indptr == X.indptr).all() and (got[0].indices == X.indices).all()
        assert (got[2] == want[2]).all() and (got[3] == want[3]).all()
        np.testing.assert_allclose(got[4], want[4], rtol=0, atol=1e-13)
        np.testing.assert_allclose(got[5], want[5], rtol=0, atol=1e-13)
    assert (Xdup.data == before).all()
