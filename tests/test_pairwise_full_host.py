"""Full-catalogue softmax of the ranking fit, host side (no device): the
NumPy restatement, the refusals before any handle, the prototypes -- and the problem and cases
of ``tests/test_hip_pairwise_full.py``."""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from test_pairwise_host import GAMMA, HYPER, _q, _small

NAMES = ("spfm_psgd_full_epoch", "spfm_psgd_full_eval")
N_CTX, N_CAND, D_CTX, D = 12, 200, 10, 24


@functools.lru_cache(maxsize=None)
def full_problem():
    """(X, Z, pairs, I, E): 12 contexts, 200 candidates (four catalogue tiles, 8 live columns in
    the last), 70 positives in a seeded order (two row tiles, 6 live rows in the second).  Context
    0: positives at 0, 63, 64, 127, 128, 199; context 1: ``exclude`` stores the whole tile
    [64, 128); context 2: ``exclude`` leaves one negative (150); contexts 3..11: 61 drawn
    positives, and ``exclude`` adds drawn non-positives to contexts 3..6."""
    rng = np.random.RandomState(3)
    X, Z = sp.lil_matrix((N_CTX, D)), sp.lil_matrix((N_CAND, D))
    for b in range(N_CTX):
        cols = rng.choice(D_CTX, size=3, replace=False)
        X[b, cols] = _q(rng.uniform(0.25, 1.0, size=3)) * np.sign(rng.randn(3))
    for c in range(N_CAND):
        cols = D_CTX + rng.choice(D - D_CTX, size=2 + c % 2, replace=False)
        Z[c, cols] = _q(rng.uniform(0.25, 1.0, size=len(cols))) * np.sign(rng.randn(len(cols)))
    pos = [(0, c) for c in (0, 63, 64, 127, 128, 199)] + [(1, 5), (1, 70), (2, 10)]
    drawn = rng.choice(9 * N_CAND, size=61, replace=False)
    pos += [(3 + int(v) // N_CAND, int(v) % N_CAND) for v in drawn]
    pairs = np.array(pos, dtype=np.int32)[rng.permutation(len(pos))]
    I = sp.csr_matrix((np.ones(len(pos)), (pairs[:, 0], pairs[:, 1])), shape=(N_CTX, N_CAND))
    E = sp.lil_matrix((N_CTX, N_CAND))
    E[1, 64:128] = 1
    E[2, [c for c in range(N_CAND) if c not in (10, 150)]] = 1
    for b in range(3, 7):
        free = np.setdiff1d(np.arange(N_CAND), I[b].indices)
        E[b, rng.choice(free, size=9, replace=False)] = 1
    return sp.csr_matrix(X), sp.csr_matrix(Z), pairs, I, sp.csr_matrix(E)


# batch 70: one minibatch; 48: a short second one.  k = 40 at degree 3: Rp = 84, two 64-column
# blocks of the gradient passes and three staging chunks of the logit product
KEYS = ("k", "degree", "fit_lower", "fit_linear", "reg", "batch", "precision")
CASES = [dict(zip(KEYS, v)) for v in [
    (3, 2, None, True, "l1", 70, "f64"), (3, 3, "explicit", True, "l21", 70, "f64"),
    (3, 3, None, False, "l1", 48, "f64"), (40, 3, None, True, "l1", 70, "f64"),
    (3, 2, None, True, "l21", 48, "f32")]]


def case_id(case):
    return "-".join(str(case[key]) for key in KEYS)


def full_params(case):
    rng = np.random.RandomState(1 + case["k"] + 7 * case["degree"])
    n_orders = case["degree"] - 1 if case["fit_lower"] == "explicit" else 1
    return (_q(0.25 * rng.randn(n_orders, case["k"], D)), _q(0.1 * rng.randn(D)),
            np.sign(rng.randn(case["k"])))


@functools.lru_cache(maxsize=None)
def _restated(ci, batch, n_epochs):
    """(F, [(P, w, sum_loss, it) after each epoch]) by the restatement; shared: read-only"""
    from sparsepoly_amd.pairwise import _forbidden, restate_full_epoch

    case = CASES[ci]
    X, Z, pairs, I, E = full_problem()
    F = _forbidden(I, E, N_CTX, N_CAND)[1]
    P, w, lams = full_params(case)
    it, out = 1, []
    for _ in range(n_epochs):
        P, w, sl, it = restate_full_epoch(
            P, w, lams, X, Z, pairs, F, case["degree"], case["reg"], gamma=GAMMA[case["reg"]],
            batch_size=batch, fit_linear=case["fit_linear"], it=it, **HYPER)
        out.append((P, w, float(sl), it))
    return F, out


def restate_case(case, batch=None, n_epochs=1):
    return _restated(CASES.index(case), case["batch"] if batch is None else batch, n_epochs)


def _wide_loss(P, w, lams, X, Z, pairs, F, degree):
    """the summed loss from dense scores in longdouble, written out independently"""
    from sparsepoly_amd.pairwise import _dense_sides, _rows_output

    Xd, Zd = _dense_sides(X, Z, np.longdouble)
    forb = F.toarray() != 0
    tot = np.longdouble(0)
    for b, c in pairs:
        s = _rows_output(P, lams.astype(np.longdouble), Xd[b][None, :] + Zd, degree)[0] + Zd @ w
        keep = ~forb[b] | (np.arange(len(s)) == c)
        tot += np.log(np.exp(s[keep] - s[keep].max()).sum()) + s[keep].max() - s[c]
    return tot


@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("degree,fit_lower", [(2, None), (3, None), (3, "explicit")])
def test_restated_gradient_equals_central_differences(degree, fit_lower, fit_linear):
    """central differences in longdouble, every coordinate of P and w.  h = 1e-5: truncation
    h^2 f''' / 6 ~ 1e-9 at third derivatives of order 10, rounding eps / h ~ 1e-14; the bar of the
    in-batch and list gradients' tests, 1e-7 of the gradient's scale, is two orders above both"""
    from sparsepoly_amd.pairwise import restate_full_gradient

    X, Z, t, P, w, lams = _small(fit_lower, fit_linear, degree, 3)
    pairs = t[:, :2]   # F: the positives and one more entry per even context
    F = sp.csr_matrix((np.ones(12), (np.r_[pairs[:, 0], 0, 2, 4], np.r_[pairs[:, 1], 1, 3, 0])),
                      shape=(6, 5))
    val, gP, gw = restate_full_gradient(P, w, lams, X, Z, pairs, F, degree)
    Pw, ww = P.astype(np.longdouble), w.astype(np.longdouble)
    f = lambda P_, w_: _wide_loss(P_, w_, lams, X, Z, pairs, F, degree)
    np.testing.assert_allclose(val.sum(), float(f(Pw, ww)), rtol=1e-12)
    h = np.longdouble(1e-5)

    def central(g, a):
        out = np.zeros(a.shape)
        for idx in np.ndindex(*a.shape):
            e = np.zeros(a.shape, dtype=np.longdouble)
            e[idx] = h
            out[idx] = float((g(a + e) - g(a - e)) / (2 * h))
        return out

    scale = max(1.0, np.abs(gP).max())
    np.testing.assert_allclose(gP, central(lambda P_: f(P_, ww), Pw), rtol=0, atol=1e-7 * scale)
    np.testing.assert_allclose(gw, central(lambda w_: f(Pw, w_), ww), rtol=0, atol=1e-7 * scale)


def test_empty_forbidden_sets_give_the_softmax_lists_over_the_whole_catalogue():
    from sparsepoly_amd.pairwise import restate_full_gradient, restate_list_gradient

    X, Z, _, P, w, lams = _small("explicit", True, 3, 3)
    pairs = np.array([[0, 0], [1, 1], [2, 4], [3, 1]], dtype=np.int32)
    F = sp.csr_matrix((np.ones(4), (pairs[:, 0], pairs[:, 1])), shape=(6, 5))
    t = np.array([(b, c, o) for b, c in pairs for o in range(5) if o != c], dtype=np.int32)
    val, gP, gw = restate_full_gradient(P, w, lams, X, Z, pairs, F, 3)
    lval, lP, lw = restate_list_gradient(P, w, lams, X, Z, t, 4, 3, "softmax")
    np.testing.assert_allclose(val, lval, rtol=1e-12)
    np.testing.assert_allclose(gP, lP, rtol=0, atol=1e-12 * np.abs(lP).max())
    np.testing.assert_allclose(gw, lw, rtol=0, atol=1e-12 * np.abs(lw).max())


@pytest.mark.parametrize("kwargs,match", [
    (dict(objective="pairwise"), "objective='softmax'"),
    (dict(objective="list"), "objective='softmax'"),
    (dict(n_negatives=2), "n_negatives must be 1"),
    (dict(proposal="popularity"), "proposal"),
    (dict(sample_weight=np.ones(3)), "sample_weight"),
    (dict(interactions=None, triples=np.array([[0, 1, 2]])), "not triples"),
    (dict(exclude=sp.csr_matrix(1 - np.eye(3))), "stores every candidate"),
    (dict(deterministic=True), "deterministic=True"),
])
def test_ranker_refuses_before_any_handle(kwargs, match, monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker, pairwise

    def boom(self):
        raise RuntimeError("reached the engine")

    monkeypatch.setattr(pairwise._BaseSparseFactorizationMachine, "_new_engine", boom)
    X = sp.csr_matrix(np.eye(3, 6))
    Z = sp.csr_matrix(np.eye(3, 6, k=3))
    kwargs = dict(kwargs)
    est = SparseFactorizationMachineRanker(regularizer="l1")
    est.deterministic = kwargs.pop("deterministic", False)
    args = dict(interactions=sp.csr_matrix(np.eye(3)), sampler="full", objective="softmax")
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        est.fit(X, Z, **args)
    est.deterministic = False
    with pytest.raises(RuntimeError, match="reached the engine"):   # the route itself: no refusal
        est.fit(X, Z, interactions=sp.csr_matrix(np.eye(3)), sampler="full", objective="softmax",
                exclude=sp.csr_matrix(np.eye(3, k=1)))


@pytest.mark.parametrize("name", NAMES)
def test_entry_is_declared_and_listed(name):
    from sparsepoly_amd import _capi

    with open(os.path.join(ROOT, "include", "spfm.h")) as f:
        assert re.search(r"^int %s\(spfm_handle h, " % name, f.read(), re.M)
    assert name in _capi.SYMBOLS
