"""Listwise ranking fit, host side (no device): the NumPy restatement
against central differences, the identity the kernel rests on, the two oracles the restatement
has (the pair gradient at M = 1, the pairwise epoch for ``'list'``), the argument errors, the
prototypes, and the near-tie cap of every case ``tests/test_hip_pairwise_list.py`` runs (it
imports its problem and its cases from here)."""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from test_pairwise_host import D, D_CTX, GAMMA, HYPER, N_CAND, N_CTX, _q, _small, pair_problem

# ---------------------------------------------------------------- the device tests' problem
N_LISTS = 60
# no list of a device case may have its positive closer than this to its best negative (lists of
# the context without a stored entry apart): 1e3 times the f64 bar of the device scores
TIE_CAP = 1e-6


def _case(k, degree, fit_lower, fit_linear, reg, objective, loss, M, batch, precision="f64",
          n_lists=N_LISTS):
    return dict(k=k, degree=degree, fit_lower=fit_lower, fit_linear=fit_linear, reg=reg,
                objective=objective, loss=loss, M=M, batch=batch, precision=precision,
                n_lists=n_lists)


# the three lane widths (k = 8, 30, 64) and component chunks (k = 70); degree 2, 3, 4; two
# orders; fit_linear on and off; the four regularizers; 'softmax' and 'list' with the three
# losses; M = 1, 3, 4, 5 (M + 1 = 4, 5: either side of a candidate batch) and 63 (the cap, at
# 4, 2 and 1 score registers per lane); batch sizes 1, 7 (60 = 8 * 7 + 4: a short last batch) and
# one batch; f64 and f32 handles; a list count shorter than one group block
CASES = [
    _case(8, 2, None, True, "l1", "softmax", "logistic", 3, 7),
    _case(30, 2, None, True, "l21", "list", "logistic", 4, 60),
    _case(64, 3, None, True, "squaredl12", "list", "squared_hinge", 5, 7),
    _case(70, 2, None, False, "squaredl21", "list", "squared", 1, 7),
    _case(8, 3, "explicit", True, "l1", "softmax", "logistic", 4, 1),
    _case(30, 4, None, True, "l1", "softmax", "logistic", 63, 60),
    _case(30, 2, None, True, "l1", "softmax", "logistic", 5, 7, precision="f32"),
    _case(70, 3, "explicit", True, "l21", "softmax", "logistic", 3, 7, precision="f32"),
    _case(8, 2, None, True, "l1", "list", "logistic", 3, 7, n_lists=10),
    _case(8, 2, None, False, "l1", "list", "squared_hinge", 63, 7),
    _case(64, 2, None, True, "squaredl12", "softmax", "logistic", 63, 60),
]


def case_id(case):
    return "k%d-deg%d-%s-lin%d-%s-%s-%s-M%d-b%d-%s-q%d" % (
        case["k"], case["degree"], case["fit_lower"], case["fit_linear"], case["reg"],
        case["objective"], case["loss"], case["M"], case["batch"], case["precision"],
        case["n_lists"])


def case_orders(case):
    return case["degree"] - 1 if case["fit_lower"] == "explicit" else 1


def list_problem(M, n_lists=N_LISTS, seed=0):
    """(X, Z, triples): the contexts and candidates of ``pair_problem`` (context 0 and candidate
    0 without an entry, context 1 with 70 entries, candidates 1 and 2 sharing attribute column
    97) and ``n_lists`` lists of ``M`` negatives, grouped.  The first lists are fixed: the empty
    context; the empty candidate as positive and as negative; the long context; a negative that
    shares an attribute column with the positive; a negative drawn twice (M >= 2)."""
    X, Z, _ = pair_problem()
    rng = np.random.RandomState(100 + seed)
    b = rng.randint(1, N_CTX, n_lists)
    cp = rng.randint(0, N_CAND, n_lists)
    neg = (cp[:, None] + rng.randint(1, N_CAND, (n_lists, M))) % N_CAND
    b[:6] = [0, 5, 5, 1, 2, 7]
    cp[:6] = [3, 0, 6, 3, 1, 9]
    neg[2, 0] = 0
    neg[4, 0] = 2
    if M >= 2:
        neg[5, :2] = 11
    neg[:6] = np.where(neg[:6] == cp[:6, None], (cp[:6, None] + 1) % N_CAND, neg[:6])
    t = np.stack([np.repeat(b, M), np.repeat(cp, M), neg.ravel()], axis=1).astype(np.int32)
    return X, Z, t


def _draw_params(case, seed):
    rng = np.random.RandomState(seed)
    P0 = _q(0.25 * rng.randn(case_orders(case), case["k"], D))
    w0 = _q(0.1 * rng.randn(D))
    return P0, w0, np.sign(rng.randn(case["k"]))


def tie_gap(P, w, lams, X, Z, t, case):
    """min over the lists (the empty context's apart) of |s_0 - max_{i>=1} s_i|"""
    from sparsepoly_amd.pairwise import restate_list_scores

    s = restate_list_scores(P, w, lams, X, Z, t, case["M"], case["degree"])
    keep = np.diff(sp.csr_matrix(X).indptr)[t[::case["M"], 0]] > 0
    return np.abs(s[:, 0] - s[:, 1:].max(axis=1))[keep].min()


@functools.lru_cache(maxsize=None)
def _restated(ci, n_epochs):
    from sparsepoly_amd.pairwise import restate_list_epoch

    case = CASES[ci]
    X, Z, t = list_problem(case["M"], case["n_lists"])
    seed = 1 + case["k"] + 7 * case["degree"]
    while True:  # reseed until the near-tie cap holds at every parameter set the tests visit
        P0, w0, lams = _draw_params(case, seed)
        P, w, it, out = P0, w0, 1, []
        ok = tie_gap(P, w, lams, X, Z, t, case) >= TIE_CAP
        for _ in range(n_epochs):
            with np.errstate(all="ignore"):  # (a draw whose epochs do not stay finite is no draw)
                P, w, sl, it = restate_list_epoch(
                    P, w, lams, X, Z, t, case["M"], case["degree"], case["objective"],
                    case["loss"], case["reg"], gamma=GAMMA[case["reg"]],
                    batch_size=case["batch"], fit_linear=case["fit_linear"], it=it, **HYPER)
                out.append((P, w, float(sl), it))
                ok = ok and tie_gap(P, w, lams, X, Z, t, case) >= TIE_CAP
        if ok:
            return (X, Z, t, P0, w0, lams), out
        seed += 1000


def restate_case(case, n_epochs=2):
    """((X, Z, triples, P0, w0, lams), [(P, w, sum_loss, it) after each epoch]) of a case by the
    restatement; computed once per process and shared -- treat every array as read-only"""
    return _restated(CASES.index(case), n_epochs)


# ---------------------------------------------------------------- 1. the restated gradient
def _small_lists(fit_lower, fit_linear, degree, M, seed=3):
    """``_small`` of the pair tests with its first four positives made lists of M negatives"""
    X, Z, t, P, w, lams = _small(fit_lower, fit_linear, degree, seed)
    rng = np.random.RandomState(seed + M)
    C = Z.shape[0]
    head = t[:4, :2]
    neg = (head[:, 1:2] + rng.randint(1, C, (4, M))) % C
    tl = np.stack([np.repeat(head[:, 0], M), np.repeat(head[:, 1], M), neg.ravel()], axis=1)
    return X, Z, tl.astype(np.int32), P, w, lams


OBJECTIVES = [("softmax", "logistic"), ("list", "logistic"), ("list", "squared_hinge"),
              ("list", "squared")]


# the gradient test's grid: objective x degree x fit_lower x fit_linear in full, M = 1, 3, 5
# rotating over it; the one list the parametrised test and the coverage check below both read
_LOWERS = (None, "explicit", "augment")
GRAD_GRID = [(oi, degree, _LOWERS[fl], lin, (1, 3, 5)[(oi + degree + fl + int(lin)) % 3])
             for oi in range(4) for degree in (2, 3, 4) for fl in range(3)
             for lin in (True, False)]


def _grid_id(g):
    return "%s-%s-deg%d-%s-lin%d-M%d" % (OBJECTIVES[g[0]] + (g[1], g[2], g[3], g[4]))


@pytest.mark.parametrize("grid", GRAD_GRID, ids=_grid_id)
def test_restated_list_gradient_equals_central_differences(grid):
    """central differences in longdouble on the restated summed loss, every coordinate of P and w,
    to the bar of the pair gradient's test (h = 1e-5: truncation ~ 1e-9, rounding ~ 1e-14)."""
    from sparsepoly_amd.pairwise import (_list_coefs, restate_list_gradient, restate_list_scores)

    oi, degree, fit_lower, fit_linear, M = grid
    objective, loss = OBJECTIVES[oi]
    X, Z, t, P, w, lams = _small_lists(fit_lower, fit_linear, degree, M)
    val, gP, gw = restate_list_gradient(P, w, lams, X, Z, t, M, degree, objective, loss)

    def f(P_, w_):
        s = restate_list_scores(P_, w_, lams, X, Z, t, M, degree, wide=True)
        return _list_coefs(s, objective, loss)[0].sum()

    np.testing.assert_allclose(val.sum(), float(f(P, w)), rtol=1e-12)
    h = np.longdouble(1e-5)
    Pw, ww = P.astype(np.longdouble), w.astype(np.longdouble)
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
    np.testing.assert_allclose(gP, fdP, rtol=0, atol=1e-7 * scale)
    np.testing.assert_allclose(gw, fdw, rtol=0, atol=1e-7 * scale)


def test_the_gradient_grid_covers_what_it_says():
    """read off GRAD_GRID itself, the list the test above is parametrised over"""
    assert len(GRAD_GRID) == 72 == len(set(g[:4] for g in GRAD_GRID))
    for dims in ((0, 4), (1, 4), (2, 4), (3, 4)):     # every objective, degree, fit_lower and
        seen = {tuple(g[i] for i in dims) for g in GRAD_GRID}   # fit_linear meets every M
        assert len(seen) == 3 * len({g[dims[0]] for g in GRAD_GRID}), dims


# ---------------------------------------------------------------- 2. invariants
def test_context_columns_of_grad_w_are_exactly_zero():
    from sparsepoly_amd.pairwise import restate_list_gradient

    case = CASES[1]
    (X, Z, t, P, w, lams), _ = restate_case(case)
    for objective, loss in OBJECTIVES:
        _, _, gw = restate_list_gradient(P, w, lams, X, Z, t, case["M"], 2, objective, loss)
        assert np.all(gw[:D_CTX] == 0.0) and np.abs(gw[D_CTX:]).max() > 0


@pytest.mark.parametrize("degree", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("objective", ["softmax", "list"])
def test_the_identity_one_recurrence_on_the_combined_array(degree, objective):
    """for every context column: dprev_1 = x * abar[0] with abar[0] taken as exactly 0,
    dprev_{t+1} = x (abar[t] - p dprev_t) on abar = sum_i coef_i a^(i) equals the sum over the
    candidates of coef_i D_j(a^(i)), to 1e-12 relative"""
    from sparsepoly_amd.pairwise import (_anova_rows, _dense_sides, _list_candidates, _list_coefs,
                                         restate_list_scores)

    M = 5
    X, Z, t, P, w, lams = _small_lists(None, True, degree, M, seed=5)
    Xd, Zd = _dense_sides(X, Z, np.double)
    b, cand = _list_candidates(t, M)
    s = restate_list_scores(P, w, lams, X, Z, t, M, degree)
    _, coef = _list_coefs(s, objective, "logistic")
    assert np.abs(coef.sum(axis=1)).max() < 1e-15
    Po = P[0]
    direct = np.zeros((len(b),) + Po.shape)
    abar = [np.zeros((len(b), Po.shape[0])) for _ in range(degree + 1)]
    for i in range(M + 1):
        V = Xd[b] + Zd[cand[:, i]]
        a = _anova_rows(Po, V, degree)
        x = Xd[b][:, None, :]                      # context columns only
        dprev = np.broadcast_to(x, direct.shape)
        for tt in range(1, degree):
            dprev = x * (a[tt][:, :, None] - Po[None] * dprev)
        direct += coef[:, i, None, None] * dprev
        for tt in range(degree + 1):
            abar[tt] = abar[tt] + coef[:, i, None] * a[tt]
    x = Xd[b][:, None, :]
    dprev = np.zeros(direct.shape)                 # x * abar[0], abar[0] := 0
    for tt in range(1, degree):
        dprev = x * (abar[tt][:, :, None] - Po[None] * dprev)
    assert np.abs(direct).max() > 1e-4
    np.testing.assert_allclose(dprev, direct, rtol=0, atol=1e-12 * np.abs(direct).max())


def test_softmax_with_one_negative_is_the_logistic_pair():
    from sparsepoly_amd.pairwise import (restate_list_gradient, restate_margins,
                                         restate_pair_gradient)

    X, Z, t, P, w, lams = _small_lists("explicit", True, 3, 1)
    val, gP, gw = restate_list_gradient(P, w, lams, X, Z, t, 1, 3, "softmax")
    pv, pP, pw = restate_pair_gradient(P, w, lams, X, Z, t, 3, "logistic")
    m = restate_margins(P, w, lams, X, Z, t, 3)
    np.testing.assert_allclose(val, np.log1p(np.exp(-m)), rtol=1e-12)
    np.testing.assert_allclose(val, pv, rtol=1e-12)
    np.testing.assert_allclose(gP, pP, rtol=0, atol=1e-12 * np.abs(pP).max())
    np.testing.assert_allclose(gw, pw, rtol=0, atol=1e-12 * np.abs(pw).max())


@pytest.mark.parametrize("loss", ["logistic", "squared_hinge", "squared"])
def test_list_epoch_is_the_pairwise_epoch_over_B_times_M_triples(loss):
    from sparsepoly_amd.pairwise import restate_list_epoch, restate_pairwise_epoch

    M, B = 3, 7
    X, Z, t = list_problem(M, 24)
    P0, w0, lams = _draw_params(CASES[0], 11)
    kw = dict(loss=loss, regularizer="l1", gamma=0.003, fit_linear=True, it=3, **HYPER)
    a = restate_list_epoch(P0, w0, lams, X, Z, t, M, 2, "list", batch_size=B, **kw)
    b = restate_pairwise_epoch(P0, w0, lams, X, Z, t, 2, batch_size=B * M, **kw)
    assert a[3] == b[3] == 3 + 4
    np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a[1], b[1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a[2] * M, b[2], rtol=1e-12)


def test_softmax_is_finite_at_scores_near_800():
    from sparsepoly_amd.pairwise import _list_coefs

    s = np.array([[800.0, -800.0, 799.0, 0.0], [-800.0, 800.0, 800.0, -799.0],
                  [800.0, 800.0, 800.0, 800.0]])
    val, coef = _list_coefs(s, "softmax", "logistic")
    assert np.isfinite(val).all() and np.isfinite(coef).all()
    np.testing.assert_allclose(coef.sum(axis=1), 0, atol=1e-15)
    np.testing.assert_allclose(val, [np.log1p(np.exp(-1.0)), 1600 + np.log(2), np.log(4)],
                               rtol=1e-12)


def test_a_duplicated_negative_counts_twice():
    """a list (c, c, c'): the loss is -s_0 + log(e^{s_0} + 2 e^{s_c} + e^{s_c'}) and the gradient
    is that of the list (c, c') with c's softmax weight doubled"""
    from sparsepoly_amd.pairwise import (restate_list_gradient, restate_list_scores,
                                         restate_pair_gradient)

    X, Z, t, P, w, lams = _small_lists(None, True, 2, 3)
    dup = t[:3].copy()
    dup[1, 2] = dup[0, 2]                             # negatives (c, c, c')
    assert dup[2, 2] != dup[0, 2]
    val, gP, gw = restate_list_gradient(P, w, lams, X, Z, dup, 3, 2, "softmax")
    s = restate_list_scores(P, w, lams, X, Z, dup, 3, 2)[0]       # (s_0, s_c, s_c, s_c')
    assert s[1] == s[2]
    z = np.exp(s[0]) + 2 * np.exp(s[1]) + np.exp(s[3])
    np.testing.assert_allclose(val[0], -s[0] + np.log(z), rtol=1e-13)
    # the gradient: sum_i pi_i grad s_i - grad s_0 with pi_c = 2 e^{s_c} / z, built from the
    # gradients of the score DIFFERENCES s_0 - s_i, which the squared pair loss hands out
    # (loss (m - 1)^2 / 2 has dloss = m - 1: one triple at a time, gradient / (m - 1) = grad m)
    want_P, want_w = np.zeros_like(gP), np.zeros_like(gw)
    for r, si, pi in ((0, s[1], 2 * np.exp(s[1]) / z), (2, s[3], np.exp(s[3]) / z)):
        _, g_m, g_mw = restate_pair_gradient(P, w, lams, X, Z, dup[r:r + 1], 2, "squared")
        m = s[0] - si
        want_P -= pi * g_m / (m - 1)                  # d(-s_0 + lse)/d theta = -sum_i pi_i grad m_i
        want_w -= pi * g_mw / (m - 1)
    assert np.abs(want_P).max() > 1e-3
    np.testing.assert_allclose(gP, want_P, rtol=0, atol=1e-12 * np.abs(want_P).max())
    np.testing.assert_allclose(gw, want_w, rtol=0, atol=1e-12 * max(np.abs(want_w).max(), 1))
    # and it is not the list with c once
    single = np.delete(dup, 1, axis=0)
    v1, g1, _ = restate_list_gradient(P, w, lams, X, Z, single, 2, 2, "softmax")
    z1 = np.exp(s[0]) + np.exp(s[1]) + np.exp(s[3])
    np.testing.assert_allclose(v1[0], -s[0] + np.log(z1), rtol=1e-13)
    assert val[0] > v1[0] and np.abs(gP - g1).max() > 1e-6


def test_epoch_lists_keeps_lists_whole_and_follows_its_rng():
    """``epoch_lists``: every epoch's triples pass ``check_lists``; with ``shuffle`` the lists are
    permuted as wholes (the same multiset of lists, rows of a list in their drawn order); the
    stream of ``rng`` is ``sample_triples`` then ``permutation(Q)`` per epoch; explicit triples
    are never redrawn"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd.pairwise import check_lists, epoch_lists, sample_triples

    M = 3
    X, Z, t = list_problem(M, 20)
    I = sp.csr_matrix((np.ones(20), (t[::M, 0], t[::M, 1])), shape=(N_CTX, N_CAND))
    I.sum_duplicates()
    Q = I.nnz
    got = list(epoch_lists(check_random_state(5), 3, interactions=I, n_negatives=M, shuffle=True))
    again = list(epoch_lists(check_random_state(5), 3, interactions=I, n_negatives=M,
                             shuffle=True))
    rng = check_random_state(5)
    for ep, out in enumerate(got):
        assert out.dtype == np.int32 and out.shape == (Q * M, 3)
        check_lists(out, M, "softmax")
        np.testing.assert_array_equal(out, again[ep])
        drawn = sample_triples(I, M, rng)
        perm = rng.permutation(Q)
        np.testing.assert_array_equal(out, drawn.reshape(Q, M, 3)[perm].reshape(-1, 3))
    assert not np.array_equal(got[0], got[1])
    # resample=False: one draw, a new permutation of the same lists per epoch
    fixed = list(epoch_lists(check_random_state(5), 3, interactions=I, n_negatives=M,
                             resample=False, shuffle=True))
    key = lambda a: sorted(map(tuple, a.reshape(-1, 3 * M)))
    assert key(fixed[0]) == key(fixed[1]) == key(fixed[2])
    assert not np.array_equal(fixed[0], fixed[1])
    # explicit triples: as given without shuffle, whole lists permuted with it
    plain = list(epoch_lists(check_random_state(1), 2, triples=t, n_negatives=M))
    assert all(np.array_equal(p, t) for p in plain)
    mixed = list(epoch_lists(check_random_state(1), 2, triples=t, n_negatives=M, shuffle=True))
    for out in mixed:
        check_lists(out, M, "list")
        assert key(out) == key(t) and not np.array_equal(out, t)


# ---------------------------------------------------------------- 3. argument errors
def test_list_argument_errors_come_before_any_handle(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker, engine
    from sparsepoly_amd import pairwise

    def boom(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", boom)
    monkeypatch.setattr(pairwise._BaseSparseFactorizationMachine, "_new_engine", boom)
    X, Z, t = list_problem(3)
    I = sp.csr_matrix((np.ones(len(t)), (t[:, 0], t[:, 1])), shape=(N_CTX, N_CAND))
    R = SparseFactorizationMachineRanker
    mixed = t[np.random.RandomState(0).permutation(len(t))]
    for objective in ("list", "softmax"):
        with pytest.raises(ValueError, match="grouped"):
            R().fit(X, Z, triples=mixed, n_negatives=3, objective=objective)
        with pytest.raises(ValueError, match="multiple of n_negatives"):
            R().fit(X, Z, triples=t[:-1], n_negatives=3, objective=objective)
        for bad in (64, 0, 2.5):
            with pytest.raises(ValueError, match="n_negatives"):
                R().fit(X, Z, interactions=I, n_negatives=bad, objective=objective)
        with pytest.raises(ValueError, match="n_negatives"):
            R().fit(X, Z, interactions=I, n_negatives=64, objective=objective,
                    sampler="dynamic")
    with pytest.raises(ValueError, match="objective"):
        R().fit(X, Z, triples=t, n_negatives=3, objective="warp")
    est = R()
    est.P_, est.w_, est.lams_ = np.zeros((1, 2, D)), np.zeros(D), np.ones(2)
    with pytest.raises(ValueError, match="grouped"):
        est.list_loss(X, Z, mixed, 3)
    with pytest.raises(ValueError, match="objective"):
        est.list_loss(X, Z, t, 3, objective="pairwise")


# ---------------------------------------------------------------- 4. prototypes
def test_header_capi_and_library_agree_on_the_list_symbols():
    import ctypes as C

    from sparsepoly_amd import _capi

    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    assert re.search(r"#define SPFM_LIST_MAX_NEG %d\b" % _capi.LIST_MAX_NEG, header)
    assert re.search(r"#define SPFM_LIST_SOFTMAX %d\b" % _capi.LIST_LOSSES["softmax"], header)
    assert re.search(r"#define SPFM_LIST_PAIRMEAN %d\b" % _capi.LIST_LOSSES["list"], header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"spfm_handle": C.c_void_p, "int": C.c_int, "double": C.c_double,
             "int64_t": C.c_int64, "const int32_t*": _capi._ip, "int64_t*": _capi._lp,
             "double*": _capi._dp}
    lib = _capi.load()
    for name in ("spfm_psgd_lists_epoch", "spfm_psgd_lists_epoch_sampled",
                 "spfm_psgd_lists_eval"):
        m = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        types = [ctype[re.sub(r"\s*\w+$", "", a).replace(" *", "*")] for a in args]
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == types, name


# ---------------------------------------------------------------- 5. the near-tie cap
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_no_list_of_a_device_case_is_a_near_tie(case):
    """at the initial parameters and after each of the two restated epochs no list has
    |s_0 - max_i s_i| < 1e-6 -- the lists of the context without a stored entry apart, the only
    ones the device comparison of the first-place flag may skip -- while the score differences are
    O(0.1), so that the cap is far from what the parameters' bar can move"""
    from sparsepoly_amd.pairwise import restate_list_scores

    (X, Z, t, P0, w0, lams), out = restate_case(case)
    assert t.shape == (case["n_lists"] * case["M"], 3)
    empty = np.diff(sp.csr_matrix(X).indptr)[t[::case["M"], 0]] == 0
    assert empty.sum() == 1 and empty[0]
    for P, w in [(P0, w0)] + [(o[0], o[1]) for o in out]:
        s = restate_list_scores(P, w, lams, X, Z, t, case["M"], case["degree"])
        assert np.isfinite(s).all()
        gap = np.abs(s[:, 0] - s[:, 1:].max(axis=1))
        assert gap[~empty].min() >= TIE_CAP, gap[~empty].min()
        assert 0.01 < np.median(gap) < 10, np.median(gap)
