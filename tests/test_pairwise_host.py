"""Pairwise ranking fit, host side (no device): the NumPy restatement against independent
gradients, its invariants, ``sample_triples``, the argument errors, the prototypes, and the
separation of the margins of every case ``tests/test_hip_pairwise.py`` runs (it imports its
problem and its cases from here)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT

# ---------------------------------------------------------------- the device tests' problem
N_CTX, N_CAND = 40, 25
# context columns [0, 72); candidates: ids [72, 97), attributes [97, 112)
D_CTX, D = 72, 112
N_TRIPLES = 150
# absolute bar of the device margins / parameters on the f64 handle (tests/test_hip_psgd.py);
# every restated margin must clear zero by 1e3 times this, so that the count of ordered triples
# can be compared exactly
MARGIN_ATOL = 1e-9


def _q(v):
    """values that a float32 handle stores exactly"""
    return np.round(v * 64) / 64


def pair_problem(seed=0):
    """(X, Z, triples): 40 contexts, 25 candidates, 112 columns, 150 triples.  Context 0 and
    candidate 0 have no entry; context 1 has 70 entries (leaves the register path on its own);
    context 2 has 60 and candidates 1, 2 have 3 each (66 together); every candidate but 0 has its
    id column and attribute columns that others share."""
    rng = np.random.RandomState(seed)
    X = sp.lil_matrix((N_CTX, D))
    for b in range(N_CTX):
        n = {0: 0, 1: 70, 2: 60}.get(b, rng.randint(3, 14))
        cols = rng.choice(D_CTX, size=n, replace=False)
        X[b, cols] = _q(rng.uniform(0.25, 1.0, size=n)) * np.sign(rng.randn(n))
    Z = sp.lil_matrix((N_CAND, D))
    for c in range(1, N_CAND):
        Z[c, D_CTX + c] = 1.0
        n = 1 if c in (1, 2) else rng.randint(0, 3)
        cols = 98 + rng.choice(14, size=n, replace=False)
        Z[c, cols] = _q(rng.uniform(0.25, 1.0, size=n))
    Z[1, 97] = 0.5          # candidates 1 and 2 share an attribute column
    Z[2, 97] = 0.75
    X, Z = sp.csr_matrix(X), sp.csr_matrix(Z)
    t = np.empty((N_TRIPLES, 3), dtype=np.int32)
    t[:, 0] = rng.randint(0, N_CTX, N_TRIPLES)
    t[:, 1] = rng.randint(0, N_CAND, N_TRIPLES)
    t[:, 2] = (t[:, 1] + rng.randint(1, N_CAND, N_TRIPLES)) % N_CAND
    t[:8] = [(0, 3, 4), (5, 0, 6), (5, 6, 0), (1, 3, 4), (2, 1, 2), (2, 2, 1), (7, 1, 2),
             (1, 2, 0)]
    return X, Z, t


def pair_params(case, seed=1):
    rng = np.random.RandomState(seed + case["k"] + 7 * case["degree"])
    P0 = _q(0.25 * rng.randn(case_orders(case), case["k"], D))
    w0 = _q(0.1 * rng.randn(D))
    lams = np.sign(rng.randn(case["k"]))
    return P0, w0, lams


def case_orders(case):
    return case["degree"] - 1 if case["fit_lower"] == "explicit" else 1


GAMMA = {"l1": 0.003, "l21": 0.05, "squaredl12": 1e-3, "squaredl21": 2e-2}
HYPER = dict(alpha=1e-2, beta=0.5, eta0=0.05, learning_rate="optimal", power_t=0.8)


def _case(k, degree, fit_lower, fit_linear, reg, loss, batch, precision="f64",
          n_triples=N_TRIPLES):
    return dict(k=k, degree=degree, fit_lower=fit_lower, fit_linear=fit_linear, reg=reg,
                loss=loss, batch=batch, precision=precision, n_triples=n_triples)


# every lane width (k = 5, 30, 40) and component chunks (k = 70); degree 2, 3, 4; two orders;
# fit_linear on and off; the four regularizers; the three losses; batch sizes 1, 64, 47 (ragged);
# f64 and f32 handles; a triple list shorter than one group block
CASES = [
    _case(5, 2, None, True, "l1", "logistic", 64),
    _case(30, 2, None, True, "l21", "logistic", 47),
    _case(40, 3, None, True, "squaredl12", "squared_hinge", 64),
    _case(70, 2, None, False, "squaredl21", "squared", 47),
    _case(5, 3, "explicit", True, "l1", "logistic", 1),
    _case(30, 4, None, True, "l1", "squared", 64),
    _case(40, 3, "explicit", False, "l21", "squared_hinge", 47),
    _case(30, 2, None, True, "l1", "logistic", 64, precision="f32"),
    _case(70, 3, None, True, "squaredl12", "logistic", 47, precision="f32"),
    _case(5, 2, None, True, "l1", "logistic", 64, n_triples=10),
    _case(30, 3, None, True, "squaredl21", "logistic", 150),
]


def case_id(case):
    return "k%d-deg%d-%s-lin%d-%s-%s-b%d-%s-m%d" % (
        case["k"], case["degree"], case["fit_lower"], case["fit_linear"], case["reg"],
        case["loss"], case["batch"], case["precision"], case["n_triples"])


def restate_case(case, n_epochs):
    """[(P, w, sum_loss, it) after each epoch] of a case by the restatement, plus its inputs"""
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z, t = pair_problem()
    t = t[:case["n_triples"]]
    P, w, lams = pair_params(case)
    it, out = 1, []
    for _ in range(n_epochs):
        P, w, sl, it = restate_pairwise_epoch(
            P, w, lams, X, Z, t, case["degree"], case["loss"], case["reg"],
            gamma=GAMMA[case["reg"]], batch_size=case["batch"], fit_linear=case["fit_linear"],
            it=it, **HYPER)
        out.append((P, w, float(sl), it))
    return (X, Z, t, lams), out


# ---------------------------------------------------------------- 1. the restated gradient
def _small(fit_lower, fit_linear, degree, seed):
    """a small problem through the estimator's own widening"""
    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import _prepare_pairs

    rng = np.random.RandomState(seed)
    B, C, dc, d = 6, 5, 7, 14
    X = sp.hstack([sp.random(B, dc, density=0.5, random_state=rng, data_rvs=rng.randn),
                   sp.csr_matrix((B, d - dc))]).tocsr()
    Z = sp.hstack([sp.csr_matrix((C, dc)),
                   sp.random(C, d - dc, density=0.4, random_state=rng, data_rvs=rng.randn)]).tocsr()
    est = SparseFactorizationMachineRanker(degree=degree, fit_lower=fit_lower,
                                           fit_linear=fit_linear)
    Xa, Za = _prepare_pairs(est, X, Z)
    t = np.stack([rng.randint(0, B, 9), rng.randint(0, C, 9)], axis=1)
    t = np.column_stack([t, (t[:, 1] + rng.randint(1, C, 9)) % C]).astype(np.int32)
    n_orders = degree - 1 if fit_lower == "explicit" else 1
    k = 3
    P = 0.4 * rng.randn(n_orders, k, Xa.shape[1])
    w = 0.3 * rng.randn(Xa.shape[1]) if fit_linear else np.zeros(Xa.shape[1])
    return Xa, Za, t, P, w, np.sign(rng.randn(k))


@pytest.mark.parametrize("loss", ["logistic", "squared_hinge", "squared"])
@pytest.mark.parametrize("degree", [2, 3, 4])
@pytest.mark.parametrize("fit_lower", [None, "explicit", "augment"])
@pytest.mark.parametrize("fit_linear", [True, False])
def test_restated_gradient_equals_central_differences(loss, degree, fit_lower, fit_linear):
    """central differences in longdouble on the restated batch loss, every coordinate of P and
    w.  h = 1e-5 in longdouble: truncation ~ h^2 f''' ~ 1e-9, rounding ~ 1e-19 / h = 1e-14."""
    from sparsepoly_amd.pairwise import _loss_pos, restate_margins, restate_pair_gradient

    X, Z, t, P, w, lams = _small(fit_lower, fit_linear, degree, seed=3)
    val, gP, gw = restate_pair_gradient(P, w, lams, X, Z, t, degree, loss)

    def f(P_, w_):
        return _loss_pos(loss, restate_margins(P_, w_, lams, X, Z, t, degree, wide=True))[0].sum()

    np.testing.assert_allclose(val.sum(), float(f(P, w)), rtol=1e-12)
    h = np.longdouble(1e-5)
    Pw = P.astype(np.longdouble)
    ww = w.astype(np.longdouble)
    fdP = np.zeros_like(P)
    for idx in np.ndindex(*P.shape):
        Pp, Pm = Pw.copy(), Pw.copy()
        Pp[idx] += h
        Pm[idx] -= h
        fdP[idx] = float((f(Pp, ww) - f(Pm, ww)) / (2 * h))
    fdw = np.zeros_like(w)
    for j in range(w.shape[0]):
        wp, wm = ww.copy(), ww.copy()
        wp[j] += h
        wm[j] -= h
        fdw[j] = float((f(Pw, wp) - f(Pw, wm)) / (2 * h))
    scale = max(1.0, np.abs(gP).max())
    # (squared_hinge has a kink: no triple of these problems sits within h of it)
    np.testing.assert_allclose(gP, fdP, rtol=0, atol=1e-7 * scale)
    np.testing.assert_allclose(gw, fdw, rtol=0, atol=1e-7 * scale)


# ---------------------------------------------------------------- 2. invariants
def test_context_columns_of_grad_w_are_exactly_zero_and_swap_negates_the_margin():
    from sparsepoly_amd.pairwise import restate_margins, restate_pair_gradient

    X, Z, t = pair_problem()
    P, w, lams = pair_params(CASES[5])
    for loss in ("logistic", "squared_hinge", "squared"):
        _, _, gw = restate_pair_gradient(P, w, lams, X, Z, t, 4, loss)
        assert np.all(gw[:D_CTX] == 0.0) and np.abs(gw[D_CTX:]).max() > 0
    m = restate_margins(P, w, lams, X, Z, t, 4)
    ms = restate_margins(P, w, lams, X, Z, t[:, [0, 2, 1]], 4)
    np.testing.assert_array_equal(ms, -m)


def test_wide_restatement_agrees_with_the_double_one():
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z, t = pair_problem()
    P, w, lams = pair_params(CASES[0])
    a = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, "logistic", "l1", gamma=0.003,
                               batch_size=47, **HYPER)
    b = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, "logistic", "l1", gamma=0.003,
                               batch_size=47, wide=True, **HYPER)
    assert a[3] == b[3] == 1 + 4
    np.testing.assert_allclose(a[0], b[0].astype(np.double), rtol=0, atol=1e-13)
    np.testing.assert_allclose(a[2], float(b[2]), rtol=1e-13)


# ---------------------------------------------------------------- 3. sample_triples
def test_sample_triples():
    from sparsepoly_amd import sample_triples

    rng = np.random.RandomState(0)
    B, C = 30, 12
    I = sp.random(B, C, density=0.3, random_state=rng, format="csr")
    E = sp.random(B, C, density=0.3, random_state=rng, format="csr")
    for excl in (None, E):
        t = sample_triples(I, n_negatives=3, random_state=5, exclude=excl)
        assert t.dtype == np.int32 and t.shape == (I.nnz * 3, 3)
        np.testing.assert_array_equal(t, sample_triples(I, 3, 5, excl))
        assert not np.array_equal(t, sample_triples(I, 3, 6, excl))
        Id = I.toarray() != 0
        assert Id[t[:, 0], t[:, 1]].all()
        assert not Id[t[:, 0], t[:, 2]].any()
        if excl is not None:
            assert not (E.toarray() != 0)[t[:, 0], t[:, 2]].any()
        # every positive, n_negatives times, in canonical order
        Ic = sp.csr_matrix(I)
        Ic.sort_indices()
        rows = np.repeat(np.arange(B), np.diff(Ic.indptr))
        np.testing.assert_array_equal(t[:, 0], np.repeat(rows, 3))
        np.testing.assert_array_equal(t[:, 1], np.repeat(Ic.indices, 3))
    # a nearly saturated row: its one free candidate is always found
    full = np.ones((2, 5))
    full[1, 3] = 0
    t = sample_triples(sp.csr_matrix(full[1:]), 4, 0)
    assert (t[:, 2] == 3).all()
    with pytest.raises(ValueError, match="row 0"):
        sample_triples(sp.csr_matrix(full), 1, 0)
    with pytest.raises(ValueError, match="row 1"):   # saturated by exclude alone
        sample_triples(sp.csr_matrix(np.array([[1, 0, 0, 0, 0], [1, 1, 1, 0, 1]])), 1, 0,
                       exclude=sp.csr_matrix(np.array([[0, 0, 0, 0, 0], [0, 0, 0, 1, 0]])))
    with pytest.raises(ValueError, match="n_negatives"):
        sample_triples(I, 0)


# ---------------------------------------------------------------- 4. argument errors
def test_argument_errors_come_before_any_handle(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker, engine
    from sparsepoly_amd import pairwise

    def boom(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", boom)
    monkeypatch.setattr(pairwise._BaseSparseFactorizationMachine, "_new_engine", boom)
    X, Z, t = pair_problem()
    I = sp.csr_matrix((np.ones(len(t)), (t[:, 0], t[:, 1])), shape=(N_CTX, N_CAND))
    R = SparseFactorizationMachineRanker
    with pytest.raises(ValueError, match="column 80 has stored entries"):
        Zb = sp.lil_matrix(Z)
        Zb[3, 80] = 1.0
        Xb = sp.lil_matrix(X)
        Xb[4, 80] = 1.0
        R().fit(sp.csr_matrix(Xb), sp.csr_matrix(Zb), triples=t)
    bad = t.copy()
    bad[17, 2] = bad[17, 1]
    with pytest.raises(ValueError, match="triple 17 has c\\+ == c-"):
        R().fit(X, Z, triples=bad)
    for col, val in ((0, N_CTX), (0, -1), (1, N_CAND), (2, -1)):
        bad = t.copy()
        bad[3, col] = val
        with pytest.raises(ValueError, match="out of range"):
            R().fit(X, Z, triples=bad)
    with pytest.raises(ValueError, match="shape"):
        R().fit(X, Z, triples=t[:, :2])
    with pytest.raises(ValueError, match="exactly one"):
        R().fit(X, Z)
    with pytest.raises(ValueError, match="exactly one"):
        R().fit(X, Z, interactions=I, triples=t)
    with pytest.raises(ValueError, match="shape"):
        R().fit(X, Z, interactions=I[:, :5])
    for solver in ("pcd", "pbcd"):
        with pytest.raises(ValueError, match="Solver"):
            R(solver=solver).fit(X, Z, triples=t)
    for reg in ("omegati", "omegacs"):
        with pytest.raises(ValueError, match="regularizer"):
            R(regularizer=reg).fit(X, Z, triples=t)
    with pytest.raises(ValueError, match="distributed"):
        R(distributed=True).fit(X, Z, triples=t)
    with pytest.raises(ValueError, match="Loss"):
        R(loss="nope").fit(X, Z, triples=t)
    with pytest.raises(ValueError, match="learning_rate"):
        R(learning_rate="nope").fit(X, Z, triples=t)
    with pytest.raises(ValueError, match="features"):
        R().fit(X[:, :100], Z, triples=t)
    est = R()
    assert not hasattr(est, "P_")
    assert R().loss == "logistic" and R().solver == "psgd"


# ---------------------------------------------------------------- 5. prototypes
def test_header_capi_and_library_agree_on_the_new_symbols():
    import ctypes as C

    from sparsepoly_amd import _capi

    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"spfm_handle": C.c_void_p, "int": C.c_int, "double": C.c_double,
             "int64_t": C.c_int64, "const int32_t*": _capi._ip, "int64_t*": _capi._lp,
             "double*": _capi._dp}
    lib = _capi.load()
    for name in ("spfm_psgd_pairs_epoch", "spfm_psgd_pairs_eval"):
        m = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        types = [ctype[re.sub(r"\s*\w+$", "", a).replace(" *", "*")] for a in args]
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == types, name


# ---------------------------------------------------------------- 6. separation of the margins
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restated_margins_of_every_device_case_are_clear_of_zero(case):
    """at the initial parameters and after the two restated epochs: the device test compares
    the count of ordered triples exactly, leaving out no triple"""
    from sparsepoly_amd.pairwise import restate_margins

    (X, Z, t, lams), out = restate_case(case, 2)
    P0, w0, _ = pair_params(case)
    for P, w in [(P0, w0)] + [(o[0], o[1]) for o in out]:
        m = restate_margins(P, w, lams, X, Z, t, case["degree"])
        assert np.isfinite(m).all()
        assert np.abs(m).min() > 1e3 * MARGIN_ATOL, np.abs(m).min()
