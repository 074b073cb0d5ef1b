"""Host side of the selected-interactions feature (sparsepoly_amd/interactions.py): the dense
NumPy restatement the device tests compare with, pinned to the metrics recorded from the reference
(tests/golden/g12_interactions.npz, tools/gen_golden_interactions.py), the symbol table, the
errors raised before any device call, and the arithmetic of ``support_recovery`` /
``estimation_error`` with the device calls stubbed.  No GPU needed.
"""
import numpy as np
import pytest
import scipy.sparse as sp
from conftest import load_golden
from sklearn.utils.validation import NotFittedError

FITS = ("sql12_pcd", "sql21_pbcd")
ENTRIES = ("spfm_interaction_stats", "spfm_interaction_topk", "spfm_interaction_list",
           "spfm_interaction_values", "spfm_interaction_block")


def restate(P, lams, tol=0.0, top=50, wide=False):
    """W = P^T diag(lams) P (P is (k, d)) over pairs j < j', dense: the pairs with |W| > tol
    sorted by (row, col), the sums over all pairs, and the `top` largest |W| among W != 0 by
    (|W| descending, row, column).  ``bound[j, j']`` = sum_s |p_sj p_sj'| (for error bounds).
    ``wide``: products and sums in ``np.longdouble`` (64-bit significand: the restatement's own
    error, at most (k + 2) 2^-64 of ``bound`` per entry, is 2000 times below the float64 forward
    error bound the device values are held to), values returned in that type."""
    P = np.asarray(P, dtype=np.double)
    lams = np.asarray(lams, dtype=np.double)
    d = P.shape[1]
    if wide:
        assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not wider than float64"
        act = np.flatnonzero((P != 0).any(axis=0))  # the other rows and columns are exact zeros
        Pa = P[:, act].astype(np.longdouble)
        W = np.zeros((d, d), dtype=np.longdouble)
        W[np.ix_(act, act)] = Pa.T @ (lams.astype(np.longdouble)[:, None] * Pa)
    else:
        W = P.T @ (lams[:, None] * P)
    iu = np.triu_indices(d, k=1)
    we = W[iu]
    sel = np.abs(we) > tol
    nz = we != 0
    rows, cols, vals = iu[0][nz], iu[1][nz], we[nz]
    order = np.lexsort((cols, rows, -np.abs(vals)))[:top]
    return dict(W=W, nnz=int(sel.sum()), active_features=int((P != 0).any(axis=0).sum()),
                rows=iu[0][sel].astype(np.int32), cols=iu[1][sel].astype(np.int32), vals=we[sel],
                sum_sq=np.sum(we ** 2), sum_abs=np.sum(np.abs(we)),
                max_abs=np.abs(we).max(initial=0.0),
                top_rows=rows[order].astype(np.int32), top_cols=cols[order].astype(np.int32),
                top_vals=vals[order], bound=np.abs(P).T @ np.abs(P))


def restate_metrics(P, lams, W_true):
    """The example's metrics over pairs j < j', W estimating 2 W_true."""
    r = restate(P, lams)
    iu = np.triu_indices(r["W"].shape[0], k=1)
    we, wt = r["W"][iu], np.asarray(W_true)[iu]
    sel, true = we != 0, wt != 0
    tp, fp, fn = int((sel & true).sum()), int((sel & ~true).sum()), int((~sel & true).sum())
    precision = 0.0 if tp + fp == 0 else tp / (tp + fp)
    recall = 0.0 if tp + fn == 0 else tp / (tp + fn)
    fscore = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    err = np.sqrt(np.sum((2.0 * wt - we) ** 2))
    scale = np.sqrt(np.sum((2.0 * wt) ** 2))
    return dict(error=float(err / scale), error_unscaled=float(err), fscore=fscore,
                pssr=(fp + fn) == 0, nnz=int(sel.sum()), tp=tp, fp=fp, fn=fn)


def test_fixture_is_the_examples_data():
    z = load_golden("g12_interactions.npz")
    assert z["X"].shape == (200, 100) and z["y"].shape == (200,)
    assert z["W_true"].sum() == 360.0  # the value the example prints
    assert int(z["max_iter"]) > 0
    for name in FITS:
        assert z[name + "_P"].shape == (30, 100) and z[name + "_lams"].shape == (30,)


@pytest.mark.parametrize("name", FITS)
def test_restatement_reproduces_the_fixture(name):
    z = load_golden("g12_interactions.npz")
    P, lams = z[name + "_P"], z[name + "_lams"]
    r = restate(P, lams)
    m = restate_metrics(P, lams, z["W_true"])
    for key in ("nnz", "tp", "fp", "fn"):
        assert m[key] == int(z[name + "_" + key]), key
    assert bool(m["pssr"]) == bool(z[name + "_pssr"])
    assert abs(m["error"] - float(z[name + "_error"])) <= 1e-12 * abs(float(z[name + "_error"]))
    assert abs(m["fscore"] - float(z[name + "_fscore"])) <= 1e-12
    np.testing.assert_array_equal(r["rows"], z[name + "_rows"])
    np.testing.assert_array_equal(r["cols"], z[name + "_cols"])
    # (values: a BLAS may sum the k terms in another order than the one that wrote the fixture)
    tol = 2 * (30 + 2) * 2.0 ** -53 * r["bound"][r["rows"], r["cols"]]
    assert (np.abs(r["vals"] - z[name + "_vals"]) <= tol).all()
    np.testing.assert_array_equal(r["top_rows"], z[name + "_top_rows"])
    np.testing.assert_array_equal(r["top_cols"], z[name + "_top_cols"])
    assert r["nnz"] == len(r["rows"]) == int(z[name + "_nnz"])


def test_symbol_table_lists_the_entries():
    from sparsepoly_amd import _capi

    for name in ENTRIES:
        assert name in _capi.SYMBOLS
    import os

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "spfm.h")).read()
    for name in ENTRIES:
        assert "int %s(spfm_handle h" % name in header


def _estimators():
    from sparsepoly_amd import (SparseAllSubsetsClassifier, SparseAllSubsetsRegressor,
                                SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)

    return (SparseFactorizationMachineRegressor, SparseFactorizationMachineClassifier,
            SparseAllSubsetsRegressor, SparseAllSubsetsClassifier)


@pytest.mark.parametrize("idx", range(4))
def test_not_fitted(idx):
    est = _estimators()[idx]()
    for call in (lambda: est.interaction_stats(), lambda: est.top_interactions(5),
                 lambda: est.interactions(), lambda: est.interaction_block([0, 1]),
                 lambda: est.interaction_values([0], [1])):
        with pytest.raises(NotFittedError):
            call()


@pytest.mark.parametrize("fit_lower", ["augment", None])
def test_degree3_without_an_explicit_lower_block(fit_lower):
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    est = SparseFactorizationMachineRegressor(degree=3, fit_lower=fit_lower)
    est.P_ = np.zeros((1, 2, 5))  # as after a fit; refused before any device call
    est.lams_ = np.ones(2)
    for call in (lambda: est.interaction_stats(), lambda: est.top_interactions(5),
                 lambda: est.interactions(), lambda: est.interaction_block([0, 1])):
        with pytest.raises(ValueError, match="no degree-2 block"):
            call()


def test_block_spec():
    from sparsepoly_amd import SparseAllSubsetsRegressor, SparseFactorizationMachineRegressor

    def spec(**kw):
        est = SparseFactorizationMachineRegressor(**kw)
        est.P_ = np.zeros((1, 1, 1))
        return est._interaction_block_spec("x")

    assert spec(degree=2) == (0, 0)
    assert spec(degree=3, fit_lower="explicit") == (1, 0)
    assert spec(degree=4, fit_lower="explicit") == (2, 0)
    assert spec(degree=2, fit_lower="augment", fit_linear=False) == (0, 1)
    assert spec(degree=2, fit_lower="augment", fit_linear=True) == (0, 0)
    est = SparseAllSubsetsRegressor()
    est.P_ = np.zeros((1, 1))
    assert est._interaction_block_spec("x") == (0, 0)


class _Stub(object):
    """An estimator whose device calls are answered from a dense W (upper triangle)."""

    def __init__(self, W):
        self.W = np.triu(np.asarray(W, dtype=np.double), k=1)
        self.W = self.W + self.W.T

    def interaction_stats(self, tol=0.0, include_augmented=False):
        we = self.W[np.triu_indices(self.W.shape[0], k=1)]
        return dict(nnz=int((np.abs(we) > tol).sum()), sum_sq=float(np.sum(we ** 2)))

    def interaction_values(self, rows, cols, include_augmented=False):
        return self.W[np.asarray(rows, dtype=int), np.asarray(cols, dtype=int)]

    def _interaction_support_query(self, rows, cols, include_augmented=False):
        return self.interaction_stats(0.0), self.interaction_values(rows, cols)


def _sym(d, pairs):
    W = np.zeros((d, d))
    for (i, j), v in pairs.items():
        W[i, j] = W[j, i] = v
    return W


@pytest.mark.parametrize("sparse", [False, True])
def test_support_recovery_arithmetic(sparse):
    from sparsepoly_amd.interactions import support_recovery

    conv = sp.csr_matrix if sparse else np.asarray
    Wt = _sym(6, {(0, 1): 0.5, (0, 2): 0.5, (3, 4): 0.5})
    # two of three true pairs found, one false pair
    got = support_recovery(_Stub(_sym(6, {(0, 1): 1.0, (3, 4): -2.0, (1, 5): 0.1})), conv(Wt))
    assert (got["tp"], got["fp"], got["fn"], got["nnz"]) == (2, 1, 1, 3)
    assert got["pssr"] is False
    assert got["fscore"] == pytest.approx(2 * (2 / 3) * (2 / 3) / (4 / 3), rel=1e-15)
    # exact recovery
    got = support_recovery(_Stub(2 * Wt), conv(Wt))
    assert (got["tp"], got["fp"], got["fn"], got["fscore"], got["pssr"]) == (3, 0, 0, 1.0, True)
    # nothing selected: precision 0 by convention, recall 0 -> fscore 0
    got = support_recovery(_Stub(np.zeros((6, 6))), conv(Wt))
    assert (got["tp"], got["fp"], got["fn"], got["nnz"], got["fscore"]) == (0, 0, 3, 0, 0)
    assert got["pssr"] is False
    # only false pairs: precision 0, recall 0
    got = support_recovery(_Stub(_sym(6, {(4, 5): 1.0})), conv(Wt))
    assert (got["tp"], got["fp"], got["fn"], got["fscore"]) == (0, 1, 3, 0)
    # empty true support (not met by the example): recall 0, no division
    got = support_recovery(_Stub(np.zeros((6, 6))), conv(np.zeros((6, 6))))
    assert (got["fscore"], got["pssr"]) == (0, True)


@pytest.mark.parametrize("sparse", [False, True])
def test_estimation_error_arithmetic(sparse):
    from sparsepoly_amd.interactions import estimation_error

    conv = sp.csr_matrix if sparse else np.asarray
    Wt = _sym(6, {(0, 1): 0.5, (0, 2): 0.25, (3, 4): -0.5})
    We = _sym(6, {(0, 1): 0.75, (3, 4): -1.0, (1, 5): 0.5, (2, 3): -0.25})
    # sum over j < j' of (2 Wt - We)^2: (1 - .75)^2 + (.5 - 0)^2 + 0 + .5^2 + .25^2
    want2 = 0.0625 + 0.25 + 0.0 + 0.25 + 0.0625
    scale2 = 1.0 + 0.25 + 1.0
    assert estimation_error(_Stub(We), conv(Wt), scaling=False) == pytest.approx(
        np.sqrt(want2), rel=1e-15)
    assert estimation_error(_Stub(We), conv(Wt)) == pytest.approx(np.sqrt(want2 / scale2),
                                                                  rel=1e-15)
    assert estimation_error(_Stub(2 * Wt), conv(Wt)) == 0.0
    assert estimation_error(_Stub(np.zeros((6, 6))), conv(Wt)) == pytest.approx(1.0, rel=1e-15)

    class Rounded(_Stub):  # sum_sq a hair below the support's squares: clamped, not NaN
        def interaction_stats(self, tol=0.0, include_augmented=False):
            s = _Stub.interaction_stats(self, tol)
            s["sum_sq"] = s["sum_sq"] * (1 - 1e-15)
            return s

    assert estimation_error(Rounded(2 * Wt), conv(Wt)) == 0.0


def test_metrics_match_the_dense_restatement_on_the_fixture():
    from sparsepoly_amd.interactions import estimation_error, support_recovery

    z = load_golden("g12_interactions.npz")
    for name in FITS:
        P, lams = z[name + "_P"], z[name + "_lams"]
        stub = _Stub(restate(P, lams)["W"])
        m = restate_metrics(P, lams, z["W_true"])
        got = support_recovery(stub, z["W_true"])
        for key in ("nnz", "tp", "fp", "fn", "pssr"):
            assert got[key] == m[key], key
        assert got["fscore"] == pytest.approx(m["fscore"], rel=1e-14)
        assert estimation_error(stub, z["W_true"]) == pytest.approx(m["error"], rel=1e-12)


def test_monitor_default_records_are_unchanged():
    from sparsepoly_amd.monitor import Monitor

    class Est(object):
        _validation = None

        def objective_terms(self):
            return dict(loss=1.0)

        def interaction_stats(self, tol=0.0):
            return dict(nnz=7 if tol == 0.0 else 3)

    m = Monitor()
    m(Est())
    assert "nnz_interactions" not in m.history[0]
    m = Monitor(interactions=True)
    m(Est())
    assert m.history[0]["nnz_interactions"] == 7
    m = Monitor(interactions=True, interaction_tol=0.5)
    m(Est())
    assert m.history[0]["nnz_interactions"] == 3
