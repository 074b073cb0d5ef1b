"""Objective terms, Monitor and validation set: everything that can be checked without a GPU.

``restate_terms`` is this suite's NumPy restatement of ``spfm_objective_terms`` (include/spfm.h):
it is what ``tests/test_hip_objective.py`` compares the device against, and it is itself pinned
here to the values recorded from the reference (``tests/golden/g10_reg_eval.npz``) -- for
``omegacs`` to the prox cache instead, because the reference's ``OmegaCS.eval`` reshapes where it
should transpose (the deviation documented in the header).
"""
import os
import pickle
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT, load_golden

from sparsepoly_amd import regularizer as R
from sparsepoly_amd.regularizer import _esp_table


def restate_terms(P, reg, degree):
    """The five quantities of ``spfm_objective_terms`` for a block ``P`` (k x d), float64."""
    P = np.asarray(P, dtype=np.float64)
    A = np.abs(P)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        norms = np.sqrt((P * P).sum(axis=0))          # per feature, over the components
        if reg == "l1":
            omega = A.sum()
        elif reg == "l21":
            omega = norms.sum()
        elif reg == "squaredl12":
            omega = (A.sum(axis=1) ** 2).sum()
        elif reg == "squaredl21":
            omega = norms.sum() ** 2
        elif reg == "omegati":
            if degree == -1:
                omega = np.prod(1.0 + A, axis=1).sum()
            else:
                omega = sum(_esp_table(row, degree)[degree] for row in A)
        elif reg == "omegacs":
            omega = np.prod(1.0 + norms) if degree == -1 else _esp_table(norms, degree)[degree]
        else:
            raise ValueError(reg)
        l2 = 0.5 * (P * P).sum()
    nz = P != 0
    return dict(l2=float(l2), omega=float(omega), nnz=int(nz.sum()),
                active_features=int(nz.any(axis=0).sum()),
                active_components=int(nz.any(axis=1).sum()))


def esp_tree(A, m, chunk=256):
    """e_0..e_m of every row of ``A`` (rows x n, non-negative), vectorised: the large-d form of
    ``_esp_table`` (same value up to the order of the non-negative summands).  The values are cut
    into runs of ``chunk``; every run takes the sequential recurrence (all runs at once), the
    runs' polynomials are multiplied pairwise, truncated at t^m.  A product with a zero factor
    counts as zero, so an overflowed coefficient never meets 0 * inf."""
    A = np.asarray(A, dtype=np.float64)
    rows, n = A.shape
    runs = 1
    while runs * chunk < max(n, 1):
        runs *= 2
    V = np.zeros((rows, runs * chunk))
    V[:, :n] = A
    V = V.reshape(rows, runs, chunk)
    T = np.zeros((rows, runs, m + 1))
    T[:, :, 0] = 1.0

    def mul(x, y):
        return np.where((x == 0) | (y == 0), 0.0, x * y)

    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(chunk):
            v = V[:, :, i]
            for t in range(m, 0, -1):
                T[:, :, t] += mul(T[:, :, t - 1], v)
        while T.shape[1] > 1:
            a, b = T[:, 0::2, :], T[:, 1::2, :]
            c = np.zeros_like(a)
            for t in range(m + 1):
                for i in range(t + 1):
                    c[:, :, t] += mul(a[:, :, i], b[:, :, t - i])
            T = c
    return T[:, 0, :]


def restate_terms_large(P, reg, degree):
    """``restate_terms`` with the polynomial by ``esp_tree`` (any d in reasonable time)."""
    P = np.asarray(P, dtype=np.float64)
    out = restate_terms(P, "l1" if reg in ("omegati", "omegacs") and degree > 0 else reg, degree)
    if reg == "omegati" and degree > 0:
        with np.errstate(over="ignore"):
            out["omega"] = float(esp_tree(np.abs(P), degree)[:, degree].sum())
    elif reg == "omegacs" and degree > 0:
        with np.errstate(over="ignore", under="ignore"):
            norms = np.sqrt((P * P).sum(axis=0))
        out["omega"] = float(esp_tree(norms[None], degree)[0, degree])
    return out


def restate_bound(k, d, degree):
    """Relative bound of the GPU comparison: all summands are non-negative, so each side's
    forward error is at most its operation count times the unit round-off."""
    return 4.0 * (d + k) * max(degree, 1) * 2.0 ** -53


# ------------------------------------------------------------------ 1. the three symbols
def test_header_capi_and_library_agree_on_the_new_symbols():
    from sparsepoly_amd import _capi

    names = ("spfm_objective_terms", "spfm_set_eval_csr", "spfm_eval_loss")
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS
    lib = _capi.load()
    for name in names:
        assert hasattr(lib, name), name


# ------------------------------------------------------------------ 2. Monitor
class _StubEstimator(object):
    def __init__(self, validation):
        self._validation = validation
        self.calls = 0

    def objective_terms(self):
        self.calls += 1
        return dict(loss=1.0 / self.calls, objective=2.0 / self.calls)

    def validation_loss(self):
        return 7.0


def test_monitor_records_and_never_stops_a_fit():
    from sparsepoly_amd.monitor import Monitor, callback_needs_params

    assert Monitor.needs_params is False
    mon = Monitor()
    est = _StubEstimator(validation=(1, 2))
    for i in range(5):
        assert mon(est) is None
        assert len(mon.history) == i + 1
    assert [h["iteration"] for h in mon.history] == [0, 1, 2, 3, 4]
    assert mon.history[2]["loss"] == 1.0 / 3 and mon.history[2]["validation_loss"] == 7.0
    assert not callback_needs_params(mon)
    assert callback_needs_params(lambda e: None)  # every other callback: exactly as before

    mon = Monitor(every=3)
    est = _StubEstimator(validation=None)
    for _ in range(7):
        assert mon(est) is None
    assert [h["iteration"] for h in mon.history] == [0, 3, 6] and est.calls == 3
    assert all(h["validation_loss"] is None for h in mon.history)
    mon = Monitor(validation=False)
    mon(_StubEstimator(validation=(1, 2)))
    assert mon.history[0]["validation_loss"] is None


# ------------------------------------------------------------------ 3. set_validation
def _estimators():
    from sparsepoly_amd import (SparseAllSubsetsClassifier, SparseAllSubsetsRegressor,
                                SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)

    return (SparseFactorizationMachineRegressor, SparseFactorizationMachineClassifier,
            SparseAllSubsetsRegressor, SparseAllSubsetsClassifier)


@pytest.mark.parametrize("idx", range(4))
def test_set_validation_is_private_state(idx):
    from sklearn.base import clone

    cls = _estimators()[idx]
    rng = np.random.RandomState(0)
    Xv = sp.random(20, 6, density=0.4, random_state=rng, format="csr")
    yv = np.where(rng.randn(20) > 0, 3.0, 5.0) if "Classifier" in cls.__name__ else rng.randn(20)
    est = cls()
    before = est.get_params()
    assert est.set_validation(Xv, yv) is est
    assert est.get_params() == before and "validation" not in " ".join(before)
    assert getattr(clone(est), "_validation", None) is None
    assert getattr(pickle.loads(pickle.dumps(est)), "_validation", None) is None
    assert est._validation is not None
    est.set_validation(None, None)
    assert est._validation is None


@pytest.mark.parametrize("idx", range(4))
def test_set_validation_rejects_what_fit_and_predict_reject(idx):
    cls = _estimators()[idx]
    rng = np.random.RandomState(1)
    X = sp.random(30, 6, density=0.4, random_state=rng, format="csr")
    binary = "Classifier" in cls.__name__
    y = np.where(rng.randn(30) > 0, 1.0, -1.0) if binary else rng.randn(30)
    Xbad = sp.random(10, 5, density=0.4, random_state=rng, format="csr")
    est = cls()
    est.set_validation(Xbad, y[:10])
    with pytest.raises(ValueError, match="features"):  # before any device work
        est.fit(X, y)
    assert not hasattr(est, "P_")
    if binary:
        with pytest.raises(TypeError, match="Only binary targets supported"):
            cls().set_validation(X, np.arange(30) % 3)
    else:
        with pytest.raises(ValueError):
            cls().set_validation(X, np.array(["a"] * 30))
    with pytest.raises(ValueError):
        cls().set_validation(X, y[:7])  # inconsistent lengths, as check_X_y in fit


def test_objective_terms_without_a_session_names_both_ways():
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.engine import SpfmError

    est = SparseFactorizationMachineRegressor()
    with pytest.raises(SpfmError, match="callback.*warm_start"):
        est.objective_terms()
    est.set_validation(np.eye(3), np.zeros(3))
    with pytest.raises(SpfmError, match="callback.*warm_start"):
        est.validation_loss()


# ------------------------------------------------------------------ 4. the restatement
def _blocks():
    z = load_golden("g10_reg_eval.npz")
    blocks = [("P2", None, z["P2"].T)]
    blocks += [("P3", q, z["P3"][q].T) for q in range(3)]
    return z, blocks


def _recorded(z, key, q):
    v = z[key]
    return float(v) if q is None else float(v[q])


def test_restatement_reproduces_the_reference_for_five_regularizers():
    z, blocks = _blocks()
    for name, q, P in blocks:
        for reg, key in (("l1", "l1|%s"), ("l21", "l21|%s|t0"), ("squaredl12", "squaredl12|%s|t1"),
                         ("squaredl21", "squaredl21|%s|t0")):
            got = restate_terms(P, reg, 2)["omega"]
            np.testing.assert_allclose(got, _recorded(z, key % name, q), rtol=1e-10)
        for deg in (2, 3, 4):
            got = restate_terms(P, "omegati", deg)["omega"]
            np.testing.assert_allclose(got, _recorded(z, "omegati|%s|deg%d" % (name, deg), q),
                                       rtol=1e-10)
    got = restate_terms(z["P2"].T, "omegati", -1)["omega"]
    np.testing.assert_allclose(got, float(z["omegati|P2|deg-1"]), rtol=1e-10)
    got = sum(restate_terms(z["P3"][q].T, "omegati", -1)["omega"] for q in range(3))
    np.testing.assert_allclose(got, float(z["omegati|P3|deg-1"]), rtol=1e-10)


def test_omegacs_follows_the_prox_cache_not_the_reference_eval():
    z, blocks = _blocks()
    for name, q, P in blocks:
        Pt = np.ascontiguousarray(P.T)  # (d, k) as pbcd holds it
        for deg in (2, 3, 4):
            reg = R.OmegaCS()
            reg.init_cache_pbcd(deg, Pt.shape[0], Pt.shape[1])
            reg.compute_cache_pbcd(Pt, deg)
            got = restate_terms(P, "omegacs", deg)["omega"]
            norms = np.sqrt((Pt * Pt).sum(axis=1))
            assert got == _esp_table(norms, deg)[deg]
            np.testing.assert_allclose(got, reg._cache[deg], rtol=1e-13)
            ref = _recorded(z, "omegacs|%s|deg%d" % (name, deg), q)
            assert abs(got - ref) > 1e-3 * abs(ref), (name, q, deg)  # 7 x 4: not square
            # ... and the host class restates the reference's eval as written
            np.testing.assert_allclose(R.OmegaCS().eval(Pt, deg), ref, rtol=1e-10)
    got = restate_terms(z["P2"].T, "omegacs", 2)["omega"]
    assert abs(got - 83.27) < 0.01 and abs(float(z["omegacs|P2|deg2"]) - 45.28) < 0.01


def test_restatement_counts():
    P = np.zeros((3, 5))
    P[0, 1] = 2.0
    P[2, 1] = -1.0
    P[2, 4] = 1e-200
    t = restate_terms(P, "l1", 2)
    assert (t["nnz"], t["active_features"], t["active_components"]) == (3, 2, 2)
    assert t["l2"] == 2.5 and t["omega"] == 3.0


def test_esp_tree_equals_the_sequential_table():
    rng = np.random.RandomState(3)
    for n in (1, 2, 7, 64, 65, 300, 1000):
        A = np.abs(rng.randn(3, n))
        A[1, ::3] = 0.0
        for m in range(1, 7):
            got = esp_tree(A, m)
            for r in range(3):
                np.testing.assert_allclose(got[r], _esp_table(A[r], m), rtol=restate_bound(1, n, m))
    P = rng.randn(4, 50)
    for reg, deg in (("omegati", 3), ("omegacs", 4), ("l21", 2), ("omegati", -1)):
        a, b = restate_terms(P, reg, deg), restate_terms_large(P, reg, deg)
        np.testing.assert_allclose(a["omega"], b["omega"], rtol=restate_bound(4, 50, deg))
        assert {k: v for k, v in a.items() if k != "omega"} == \
            {k: v for k, v in b.items() if k != "omega"}
