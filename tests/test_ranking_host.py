"""``sparsepoly_amd.ranking`` without a device: the NumPy restatement ``restate_scores`` against
reference-produced predictions, the decomposition the device code is built on against that
restatement, and the argument errors that are raised before any device use."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import load_golden
from sklearn.utils.validation import NotFittedError


def fm(degree, k, d, fit_lower="explicit", fit_linear=True, seed=0, cls=None, signs=True):
    """An estimator with P_, w_, lams_ assigned directly (no training), over d features."""
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    cls = cls or SparseFactorizationMachineRegressor
    rng = np.random.RandomState(seed)
    est = cls(degree=degree, n_components=k, fit_lower=fit_lower, fit_linear=fit_linear,
              precision="f64")
    n_dummy = degree - (2 if fit_linear else 1) if fit_lower == "augment" else 0
    n_orders = degree - 1 if fit_lower == "explicit" else 1
    est.P_ = rng.randn(n_orders, k, d + n_dummy) * 0.5
    est.w_ = rng.randn(d + n_dummy) if fit_linear else np.zeros(d + n_dummy)
    est.lams_ = np.where(rng.rand(k) < 0.5, -1.0, 1.0) if signs else np.ones(k)
    return est


def all_subsets(k, d, seed=0, cls=None):
    from sparsepoly_amd import SparseAllSubsetsRegressor

    rng = np.random.RandomState(seed)
    est = (cls or SparseAllSubsetsRegressor)(n_components=k, precision="f64")
    est.P_ = rng.randn(k, d) * 0.3
    est.lams_ = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    return est


def sides(B, C, d, seed=0, z_entries=3, split=None):
    """Contexts on the columns [0, split), candidates on [split, d): disjoint by construction.
    Row 0 of each side is empty when it has more than one row."""
    rng = np.random.RandomState(seed + 1000)
    split = d // 2 if split is None else split
    X = np.zeros((B, d))
    Z = np.zeros((C, d))
    for b in range(1 if B > 1 else 0, B):
        cols = rng.choice(split, size=min(split, 3 + rng.randint(3)), replace=False)
        X[b, cols] = rng.randn(len(cols))
    for c in range(1 if C > 1 else 0, C):
        cols = split + rng.choice(d - split, size=min(d - split, z_entries), replace=False)
        Z[c, cols] = rng.randn(len(cols))
    return sp.csr_matrix(X), sp.csr_matrix(Z)


def anova(PX, m):
    """a[t], t = 0..m, each (n, k), of the rows of PX (n, k, d)"""
    a = [np.ones(PX.shape[:2], dtype=PX.dtype)] + [np.zeros(PX.shape[:2], dtype=PX.dtype)
                                                   for _ in range(m)]
    for j in np.flatnonzero((PX != 0).any(axis=(0, 1))):
        for t in range(m, 0, -1):
            a[t] = a[t] + a[t - 1] * PX[:, :, j]
    return a


def decomposed(est, X, Z, dtype=np.double):
    """f(x) + f(z) + cross from the towers, the way the device code forms the scores"""
    from sparsepoly_amd.ranking import _prepare, _spec

    degree, lin, lower, P, w, lams = _spec(est)
    P, w, lams = P.astype(dtype), w.astype(dtype), lams.astype(dtype)
    Xa, Za = _prepare(est, X, Z)
    Xd, Zd = Xa.toarray().astype(dtype), Za.toarray().astype(dtype)
    if degree == -1:
        U = np.prod(1 + P[0][None] * Xd[:, None, :], axis=2) * lams
        V = np.prod(1 + P[0][None] * Zd[:, None, :], axis=2)
        return U @ V.T
    blocks = [(0, degree)] + ([(1, 2)] if lower else [])
    out = np.zeros((Xd.shape[0], Zd.shape[0]), dtype=dtype)
    for o, m in blocks:
        ax = anova(P[o][None] * Xd[:, None, :], m)
        az = anova(P[o][None] * Zd[:, None, :], m)
        out += ((ax[m] * lams).sum(axis=1))[:, None] + ((az[m] * lams).sum(axis=1))[None, :]
        for t in range(1, m):
            out += (ax[t] * lams) @ az[m - t].T
    if lin:
        out += (Xd @ w)[:, None] + (Zd @ w)[None, :]
    return out


def abs_model(est):
    """The model with every parameter replaced by its magnitude and every sign +1: on |X|, |Z| its
    score is the sum of the magnitudes of the monomials a score is made of."""
    import copy

    ab = copy.copy(est)
    ab.P_ = np.abs(est.P_)
    if hasattr(est, "w_"):
        ab.w_ = np.abs(est.w_)
    ab.lams_ = np.ones_like(est.lams_)
    return ab


@pytest.mark.parametrize("tag", ["deg2", "deg3", "deg4", "deg5", "deg2|explicit", "deg3|explicit",
                                 "deg3|None"])
def test_restatement_reproduces_the_recorded_predictions(tag):
    """With candidates that store nothing, colconst = 0 and there is no cross term: the scores
    are the recorded predictions of g6_anova.npz, at that file's own tolerance."""
    from sparsepoly_amd.ranking import restate_scores

    z = load_golden("g6_anova.npz")
    X = z["X"]
    if "|" in tag:
        deg, fl = tag.split("|")
        est = fm(int(deg[3:]), 4, X.shape[1], fit_lower=None if fl == "None" else fl)
        est.P_, est.w_, est.lams_ = z["est_P|" + tag], z["est_w|" + tag], z["lams"]
        want = z["est_pred|" + tag]
    else:
        est = fm(int(tag[3:]), 4, X.shape[1], fit_lower=None, fit_linear=False)
        est.P_, est.w_, est.lams_ = z["P"][None], np.zeros(X.shape[1]), z["lams"]
        want = z["pred|" + tag]
    Z = sp.csr_matrix((3, X.shape[1]))
    got = restate_scores(est, X, Z)
    assert got.shape == (X.shape[0], 3)
    for c in range(3):
        np.testing.assert_allclose(got[:, c], want, rtol=0, atol=1e-10)


@pytest.mark.parametrize("degree,fit_lower,fit_linear", list(itertools.product(
    (2, 3, 4, 5, 6), ("explicit", "augment", None), (True, False))))
def test_decomposition_equals_the_restatement(degree, fit_lower, fit_linear):
    from sparsepoly_amd.ranking import restate_scores

    est = fm(degree, 3, 10, fit_lower, fit_linear, seed=degree)
    X, Z = sides(5, 7, 10, seed=degree)
    want = restate_scores(est, X, Z)
    got = decomposed(est, X, Z)
    assert np.abs(want).max() > 1e-3
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))


def test_decomposition_equals_the_restatement_all_subsets():
    from sparsepoly_amd.ranking import restate_scores

    est = all_subsets(4, 10)
    X, Z = sides(5, 7, 10)
    want = restate_scores(est, X, Z)
    np.testing.assert_allclose(decomposed(est, X, Z), want, rtol=0,
                               atol=1e-12 * max(1.0, np.abs(want).max()))


def test_augmented_candidates_get_empty_dummy_columns():
    """fit_lower='augment': the dummy columns belong to the contexts; a candidate's own constant
    is the output of its widened row, not predict(Z)"""
    from sparsepoly_amd.ranking import _prepare

    est = fm(4, 2, 6, "augment", True)
    X, Z = sides(3, 4, 6)
    Xa, Za = _prepare(est, X, Z)
    n_dummy = est.P_.shape[2] - 6
    assert n_dummy == 2 and Xa.shape[1] == Za.shape[1] == 8
    dummy = np.flatnonzero(np.asarray((Xa != 0).sum(axis=0)).ravel() == Xa.shape[0])
    assert len(dummy) == n_dummy
    assert not np.isin(Za.indices, dummy).any() and Za.nnz == Z.nnz


def test_argument_errors_come_before_any_device_use(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRegressor, engine
    from sparsepoly_amd.ranking import restate_scores

    def no_device(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", no_device)
    est = fm(2, 3, 10)
    X, Z = sides(4, 6, 10)
    Xo = X.tolil()
    Xo[2, 7] = 1.5  # column 7 belongs to the candidates
    Xo = Xo.tocsr()
    assert 7 in Z.indices
    for call in (lambda: est.candidate_scores(Xo, Z), lambda: est.top_candidates(Xo, Z, 3),
                 lambda: restate_scores(est, Xo, Z)):
        with pytest.raises(ValueError, match=r"column \d+ has stored entries") as ei:
            call()
        col = int(str(ei.value).split()[1])
        assert col in Xo.indices and col in Z.indices
    with pytest.raises(ValueError, match="features"):
        est.candidate_scores(X[:, :9], Z)
    with pytest.raises(ValueError, match="features"):
        est.candidate_scores(sp.csr_matrix((2, 12)), sp.csr_matrix((3, 12)))
    with pytest.raises(ValueError, match="features"):
        est.ranker(sp.csr_matrix((3, 12)))
    for K in (0, -1):
        with pytest.raises(ValueError, match="K must be"):
            est.top_candidates(X, Z, K)
    with pytest.raises(ValueError, match="exceeds the cap"):
        est.top_candidates(X, Z, 100000)
    unfitted = SparseFactorizationMachineRegressor()
    for call in (lambda: unfitted.candidate_scores(X, Z), lambda: unfitted.top_candidates(X, Z, 1),
                 lambda: unfitted.ranker(Z)):
        with pytest.raises(NotFittedError):
            call()


def test_inputs_are_canonicalised_and_left_alone():
    """unsorted indices and duplicates: summed, and the caller's arrays are not changed"""
    from sparsepoly_amd.ranking import restate_scores

    est = fm(3, 2, 8)
    X, Z = sides(3, 4, 8)
    Xc = X.tocoo()
    rows = np.concatenate([Xc.row, Xc.row])[::-1]
    cols = np.concatenate([Xc.col, Xc.col])[::-1]
    vals = np.concatenate([0.25 * Xc.data, 0.75 * Xc.data])[::-1]
    Xdup = sp.coo_matrix((vals, (rows, cols)), shape=X.shape).tocsc()
    before = Xdup.data.copy()
    np.testing.assert_allclose(restate_scores(est, Xdup, Z), restate_scores(est, X, Z), rtol=0,
                               atol=1e-13)
    assert (Xdup.data == before).all()
