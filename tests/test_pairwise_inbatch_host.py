"""In-batch softmax of the ranking fit, host side (no device): the NumPy
restatement against central differences and against the tested list restatement, the masking
rules, the refusals before any handle, the prototypes -- and the problem and cases of
``tests/test_hip_pairwise_inbatch.py``."""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from test_pairwise_host import GAMMA, HYPER, _q, _small, pair_params, pair_problem

NAMES = ("spfm_psgd_inbatch_epoch", "spfm_psgd_inbatch_eval")


# ---------------------------------------------------------------- the device tests' problem
def inbatch_problem():
    """(X, Z, pairs): the pair tests' 40 contexts and 25 candidates (context 0 and candidate 0
    empty, context 1 with 70 entries) with column 111 stored by every other candidate, and the 150
    positives (b, c+) of its triples: contexts and candidates repeat inside every batch."""
    X, Z, t = pair_problem()
    Z = Z.tolil()
    Z[1:, 111] = _q(np.random.RandomState(5).uniform(0.25, 1.0, size=Z.shape[0] - 1))[:, None]
    return X, sp.csr_matrix(Z), np.ascontiguousarray(t[:, :2])


def _case(k, degree, fit_lower, fit_linear, reg, batch, precision="f64"):
    return dict(k=k, degree=degree, fit_lower=fit_lower, fit_linear=fit_linear, reg=reg,
                batch=batch, precision=precision)


# m = 150.  batch 64: minibatches of 64, 64, 22; 65 and 130: a second and a third tile with one
# and two live rows; 1; >= m.  k = 8 (R < 32), 30, 33 (an MFMA chunk plus a column and the ones
# column), 70 (lane groups in chunks; two 64-column blocks of the towers); two orders; degree 4
# (R = 90); both squared-norm proxes' simpler kin l1 and squaredl12; both precisions
CASES = [
    _case(8, 2, None, True, "l1", 64),
    _case(30, 2, None, True, "l1", 65, "f32"),
    _case(33, 2, None, False, "squaredl12", 130),
    _case(70, 2, None, True, "l1", 200, "f32"),
    _case(8, 3, "explicit", True, "l1", 64),
    _case(30, 4, None, True, "l1", 65),
    _case(8, 2, None, True, "l1", 1),
    _case(33, 3, "explicit", True, "squaredl12", 150, "f32"),
]


def case_id(case):
    return "k%d-deg%d-%s-lin%d-%s-b%d-%s" % (case["k"], case["degree"], case["fit_lower"],
                                             case["fit_linear"], case["reg"], case["batch"],
                                             case["precision"])


@functools.lru_cache(maxsize=None)
def _restated(ci, batch):
    from sparsepoly_amd.pairwise import restate_inbatch_epoch

    case = CASES[ci]
    X, Z, pairs = inbatch_problem()
    P0, w0, lams = pair_params(case)
    P, w, it, out = P0, w0, 1, []
    for _ in range(2):
        P, w, sl, it = restate_inbatch_epoch(
            P, w, lams, X, Z, pairs, case["degree"], case["reg"], gamma=GAMMA[case["reg"]],
            batch_size=batch, fit_linear=case["fit_linear"], it=it, **HYPER)
        out.append((P, w, float(sl), it))
    return (X, Z, pairs, P0, w0, lams), out


def restate_case(case, batch=None):
    """((X, Z, pairs, P0, w0, lams), [(P, w, sum_loss, it) after each of two epochs]) by the
    restatement; computed once per process and shared -- treat every array as read-only"""
    return _restated(CASES.index(case), case["batch"] if batch is None else batch)


# ---------------------------------------------------------------- the restated gradient
def _wide_loss(P, w, lams, X, Z, pairs, degree):
    """the summed loss from dense scores in longdouble, written out independently"""
    from sparsepoly_amd.pairwise import _dense_sides, _rows_output

    Xd, Zd = _dense_sides(X, Z, np.longdouble)
    b, c = pairs[:, 0], pairs[:, 1]
    tot = np.longdouble(0)
    for q in range(len(b)):
        s = _rows_output(P[None] if P.ndim == 2 else P, lams.astype(np.longdouble),
                         Xd[b[q]][None, :] + Zd[c], degree)[0] + Zd[c] @ w
        keep = ((b != b[q]) & (c != c[q])) | (np.arange(len(b)) == q)
        tot += np.log(np.exp(s[keep] - s[keep].max()).sum()) + s[keep].max() - s[q]
    return tot


@pytest.mark.parametrize("fit_linear", [True, False])
@pytest.mark.parametrize("fit_lower", [None, "explicit", "augment"])
@pytest.mark.parametrize("degree", [2, 3, 4])
def test_restated_gradient_equals_central_differences(degree, fit_lower, fit_linear):
    """central differences in longdouble, every coordinate of P and w, at the bar of the list
    gradient's test (h = 1e-5: truncation ~ 1e-9, rounding ~ 1e-14)"""
    from sparsepoly_amd.pairwise import restate_inbatch_gradient

    X, Z, t, P, w, lams = _small(fit_lower, fit_linear, degree, 3)
    pairs = t[:, :2]
    val, gP, gw = restate_inbatch_gradient(P, w, lams, X, Z, pairs, degree)
    Pw, ww = P.astype(np.longdouble), w.astype(np.longdouble)
    f = lambda P_, w_: _wide_loss(P_, w_, lams, X, Z, pairs, degree)
    np.testing.assert_allclose(val.sum(), float(f(Pw, ww)), rtol=1e-12)
    h = np.longdouble(1e-5)

    def central(g, a):
        out = np.zeros(a.shape)
        for idx in np.ndindex(*a.shape):
            ap, am = a.copy(), a.copy()
            ap[idx] += h
            am[idx] -= h
            out[idx] = float((g(ap) - g(am)) / (2 * h))
        return out

    fdP, fdw = central(lambda P_: f(P_, ww), Pw), central(lambda w_: f(Pw, w_), ww)
    scale = max(1.0, np.abs(gP).max())
    np.testing.assert_allclose(gP, fdP, rtol=0, atol=1e-7 * scale)
    np.testing.assert_allclose(gw, fdw, rtol=0, atol=1e-7 * scale)


def _as_lists(pairs, keep):
    """the grouped triples (b_q, c_q, c_q') over the columns q' != q with keep[q, q']; every row
    must keep the same number of them"""
    n = len(pairs)
    rows = [(pairs[q, 0], pairs[q, 1], pairs[qq, 1])
            for q in range(n) for qq in range(n) if qq != q and keep[q, qq]]
    return np.array(rows, dtype=np.int32), len(rows) // n


@pytest.mark.parametrize("rule", ["distinct", "same_candidate", "same_context"])
def test_batch_equals_the_softmax_lists_over_its_admitted_columns(rule):
    """distinct: all contexts and candidates differ and every row is the list of all others.
    same_candidate / same_context: two positions share one, and each row's list leaves the
    masked column out -- here by pairing them so that every row masks exactly one column."""
    from sparsepoly_amd.pairwise import restate_inbatch_gradient, restate_list_gradient

    X, Z, _, P, w, lams = _small("explicit", True, 3, 3)
    pairs = np.array([[0, 0], [1, 1], [2, 2], [3, 3]], dtype=np.int32)
    if rule == "same_candidate":
        pairs[:, 1] = [0, 0, 2, 2]
    if rule == "same_context":
        pairs[:, 0] = [4, 5, 5, 4]
    b, c = pairs[:, 0], pairs[:, 1]
    keep = (b[:, None] != b[None, :]) & (c[:, None] != c[None, :])
    assert keep.sum() == (12 if rule == "distinct" else 8)
    t, M = _as_lists(pairs, keep)
    val, gP, gw = restate_inbatch_gradient(P, w, lams, X, Z, pairs, 3)
    lval, lP, lw = restate_list_gradient(P, w, lams, X, Z, t, M, 3, "softmax")
    np.testing.assert_allclose(val, lval, rtol=1e-12)
    np.testing.assert_allclose(gP, lP, rtol=0, atol=1e-12 * np.abs(lP).max())
    np.testing.assert_allclose(gw, lw, rtol=0, atol=1e-12 * np.abs(lw).max())


def test_a_lone_position_has_no_loss_and_no_gradient_and_large_scores_stay_finite():
    from sparsepoly_amd.pairwise import restate_inbatch_gradient

    X, Z, t, P, w, lams = _small(None, True, 2, 3)
    pairs = t[:, :2]
    val, gP, gw = restate_inbatch_gradient(P, w, lams, X, Z, pairs[:1], 2)
    assert val[0] == 0 and not gP.any() and not gw.any()
    # a batch whose every other position is masked is n lone positions
    same = np.stack([np.full(3, pairs[0, 0]), np.arange(3)], axis=1)
    val, gP, gw = restate_inbatch_gradient(P, w, lams, X, Z, same, 2)
    assert not val.any() and not gP.any() and not gw.any()
    big = np.zeros_like(w)
    big[Z.indices] = 800.0 / np.abs(Z.data).min() * np.sign(np.arange(Z.nnz) % 2 - 0.5)
    val, gP, gw = restate_inbatch_gradient(P, big, lams, X, Z, pairs, 2)
    assert np.abs(Z @ big).max() >= 800
    assert np.isfinite(val).all() and np.isfinite(gP).all() and np.isfinite(gw).all()


# ---------------------------------------------------------------- refusals, prototypes
@pytest.mark.parametrize("kwargs,match", [
    (dict(objective="pairwise"), "objective='softmax'"),
    (dict(objective="list"), "objective='softmax'"),
    (dict(n_negatives=2), "n_negatives must be 1"),
    (dict(exclude=sp.csr_matrix((3, 3))), "exclude"),
    (dict(proposal="popularity"), "proposal"),
    (dict(sample_weight=np.ones(2)), "sample_weight"),
])
def test_ranker_refuses_before_any_handle(kwargs, match, monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker, pairwise

    def boom(self):
        raise RuntimeError("reached the engine")

    monkeypatch.setattr(pairwise._BaseSparseFactorizationMachine, "_new_engine", boom)
    X = sp.csr_matrix(np.eye(3, 6))
    Z = sp.csr_matrix(np.eye(3, 6, k=3))
    t = np.array([[0, 1, 2], [1, 0, 2]])
    est = SparseFactorizationMachineRanker(regularizer="l1")
    args = dict(triples=t, sampler="in_batch", objective="softmax")
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        est.fit(X, Z, **args)
    with pytest.raises(RuntimeError, match="reached the engine"):   # the route itself: no refusal
        est.fit(X, Z, triples=t, sampler="in_batch", objective="softmax")
    with pytest.raises(RuntimeError, match="reached the engine"):
        est.fit(X, Z, interactions=sp.csr_matrix(np.eye(3)), sampler="in_batch",
                objective="softmax")


@pytest.mark.parametrize("name", NAMES)
def test_entry_is_declared_and_listed(name):
    from sparsepoly_amd import _capi

    with open(os.path.join(ROOT, "include", "spfm.h")) as f:
        assert re.search(r"^int %s\(spfm_handle h, " % name, f.read(), re.M)
    assert name in _capi.SYMBOLS
