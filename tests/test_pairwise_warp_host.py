"""Weighted triples, proposal draws and the WARP sampler, host side (no
device): the weighted restated gradient against central differences, the quantiser and the
weighted integer draw, ``restate_warp`` against its definition, the argument errors, the
prototypes, and the coverage / near-tie conditions of every case
``tests/test_hip_pairwise_warp.py`` runs (it imports its parameters and margins from here).  The
problem, the cases and the interactions are those of ``tests/test_pairwise_host.py`` and
``tests/test_pairwise_sample_host.py``."""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from test_pairwise_host import (CASES, D, N_CAND, N_CTX, _q, _small, case_id, case_orders,
                                pair_problem)
from test_pairwise_sample_host import (FREE_CAND, FULL_CTX, M_VALUES, NEAR_TIE, NEAR_TIE_SHARE,
                                       dense_scores, forbidden_dense, sample_interactions)

WARP_SEED, WARP_EPOCH = 4242, 1


# ---------------------------------------------------------------- the device tests' parameters
def _draw_params(case, seed):
    """the draw of ``pair_params`` (and of the list tests) from an explicit seed"""
    rng = np.random.RandomState(seed)
    P0 = _q(0.25 * rng.randn(case_orders(case), case["k"], D))
    w0 = _q(0.1 * rng.randn(D))
    return P0, w0, np.sign(rng.randn(case["k"]))


def spread_margin(P, w, lams, X, Z, degree):
    """The case's second margin, from the restated score spread: minus the 0.9 quantile of
    s(b, c) - s(b, c+) over the positives and their admissible candidates, so that about one
    trial in ten violates (margin 0: about one in two)."""
    I, E = sample_interactions()
    S = dense_scores(P, w, lams, X, Z, degree).astype(np.double)
    F = forbidden_dense(I, E)
    rows = np.repeat(np.arange(N_CTX), np.diff(I.indptr))
    diff = np.concatenate([S[b][~F[b]] - S[b, c] for b, c in zip(rows, I.indices)])
    return -float(np.quantile(diff, 0.9))


def _coverage(P, w, lams, X, Z, degree, margins):
    """(the set of trial classes seen, worst near-tie share, near ties outside context 0)"""
    from sparsepoly_amd.pairwise import restate_warp

    I, E = sample_interactions()
    seen, worst, outside = set(), 0.0, 0
    for margin in margins:
        for M in M_VALUES:
            n_neg = 3 if M == 3 else 1
            t, _, wt, tr, near = restate_warp(P, w, lams, X, Z, I, degree, n_neg, M, 64 * M,
                                              margin, WARP_SEED, WARP_EPOCH, exclude=E)
            seen |= {"1"} if (tr == 1).any() else set()
            seen |= {"2-4"} if ((tr > 1) & (tr <= 4)).any() else set()
            seen |= {">4"} if (tr > 4).any() else set()
            seen |= {">16"} if (M == 33 and (tr > 16).any()) else set()
            seen |= {"0"} if (tr == 0).any() else set()
            tie = near < NEAR_TIE
            worst = max(worst, tie.mean())
            outside += int((t[tie, 0] != 0).sum())
    return seen, worst, outside


ALL_CLASSES = {"1", "2-4", ">4", ">16", "0"}


@functools.lru_cache(maxsize=None)
def _warp_case(ci):
    case = CASES[ci]
    X, Z, _ = pair_problem()
    seed = 1 + case["k"] + 7 * case["degree"]      # the seed of pair_params
    while True:  # reseed (the rule of the list tests) until the restatement covers and is capped
        P, w, lams = _draw_params(case, seed)
        margin = spread_margin(P, w, lams, X, Z, case["degree"])
        seen, worst, outside = _coverage(P, w, lams, X, Z, case["degree"], (0.0, margin))
        if seen == ALL_CLASSES and worst <= NEAR_TIE_SHARE and outside == 0:
            return P, w, lams, margin, seed
        seed += 1000


def warp_params(case):
    """(P, w, lams, the case's spread margin): the parameters the device tests of a case start
    from; computed once per process and shared -- treat every array as read-only"""
    return _warp_case(CASES.index(case))[:4]


def triple_weights():
    """the triple weights of the device tests: zeros, ones and non-integers"""
    return np.array([0.0, 1.0, 2.5, 0.375, 1.0, 0.0, 3.25, 0.0625])


# ---------------------------------------------------------------- 1. the weighted gradient
@pytest.mark.parametrize("loss", ["logistic", "squared_hinge", "squared"])
@pytest.mark.parametrize("degree", [2, 3, 4])
@pytest.mark.parametrize("fit_lower", [None, "explicit"])
def test_weighted_gradient_equals_central_differences(loss, degree, fit_lower):
    """central differences in longdouble of sum_q wt_q loss_q (h = 1e-5: truncation ~ 1e-9),
    at the bar of the unweighted test; a triple of weight 0 contributes nothing"""
    from sparsepoly_amd.pairwise import _loss_pos, restate_margins, restate_pair_gradient

    X, Z, t, P, w, lams = _small(fit_lower, True, degree, seed=3)
    wt = np.array([0.0, 1.0, 2.5, 0.375, 1.0, 0.0, 3.25, 0.0625, 1.75])
    val, gP, gw = restate_pair_gradient(P, w, lams, X, Z, t, degree, loss, weights=wt)
    plain = restate_pair_gradient(P, w, lams, X, Z, t, degree, loss)[0]
    np.testing.assert_array_equal(val, wt * plain)
    assert (val[wt == 0] == 0).all()
    # without the weight-0 triples: the same sums
    on = wt != 0
    _, gP1, gw1 = restate_pair_gradient(P, w, lams, X, Z, t[on], degree, loss, weights=wt[on])
    np.testing.assert_allclose(gP, gP1, rtol=0, atol=1e-13 * max(1.0, np.abs(gP).max()))
    np.testing.assert_allclose(gw, gw1, rtol=0, atol=1e-13 * max(1.0, np.abs(gw).max()))
    # all ones: the unweighted gradient, bit for bit
    for a, b in zip(restate_pair_gradient(P, w, lams, X, Z, t, degree, loss,
                                          weights=np.ones(len(t))),
                    restate_pair_gradient(P, w, lams, X, Z, t, degree, loss)):
        np.testing.assert_array_equal(a, b)

    wl = wt.astype(np.longdouble)

    def f(P_, w_):
        m = restate_margins(P_, w_, lams, X, Z, t, degree, wide=True)
        return (wl * _loss_pos(loss, m)[0]).sum()

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


def test_weighted_epoch_restatement_sums_weighted_losses():
    from sparsepoly_amd.pairwise import restate_pair_gradient, restate_pairwise_epoch

    X, Z, t = pair_problem()
    case = CASES[0]
    P, w, lams = _draw_params(case, 1 + case["k"] + 7 * case["degree"])
    wt = np.resize(triple_weights(), len(t))
    kw = dict(loss="logistic", regularizer="l1", gamma=0.003, batch_size=len(t))
    P1, w1, sl, it = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, weights=wt, **kw)
    assert it == 2
    np.testing.assert_allclose(
        float(sl), restate_pair_gradient(P, w, lams, X, Z, t, 2, "logistic", weights=wt)[0].sum(),
        rtol=1e-14)
    P2, w2, sl2, _ = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, **kw)
    assert not np.array_equal(P1, P2) and float(sl2) != float(sl)
    ones = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, weights=np.ones(len(t)), **kw)
    assert np.array_equal(ones[0], P2) and np.array_equal(ones[1], w2)


# ---------------------------------------------------------------- 2. the quantiser and the draw
def test_quantiser_total_positive_and_zero_weights():
    from sparsepoly_amd.pairwise import proposal_cum, quantise_proposal

    rng = np.random.RandomState(0)
    for w in (np.array([0.0, 1.0, 2.0, 0.0, 5.5]),
              np.r_[1.0, np.full(10 ** 6, 1e-30)],            # a long tail under one quantum each
              np.r_[1e300, 1e-300, 0.0, 1.0],
              rng.rand(1000) * (rng.rand(1000) < 0.7),
              (np.arange(25) + 1.0) ** 0.75,
              np.array([3.0])):
        q = quantise_proposal(w)
        assert q.dtype == np.int64 and q.shape == w.shape
        assert int(q.sum()) < 2 ** 32
        assert (q[w > 0] >= 1).all() and (q[w == 0] == 0).all()
        want = np.maximum(np.floor(w / w.sum() * 2.0 ** 31), (w > 0) * 1.0)
        np.testing.assert_array_equal(q, want.astype(np.int64))
        cum = proposal_cum(q)
        assert cum.dtype == np.uint32 and int(cum[-1]) == int(q.sum())
        assert (np.diff(cum.astype(np.int64)) >= 0).all()
    # the bound for every admissible C: floor terms sum to <= 2^31, the lifts add at most C < 2^31
    assert 2 ** 31 + (2 ** 31 - 1) < 2 ** 32
    for bad in ([1.0, -1.0], [1.0, np.nan], [np.inf, 1.0], [0.0, 0.0], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="proposal"):
            quantise_proposal(bad)
    with pytest.raises(ValueError, match="proposal"):
        quantise_proposal([1.0, 2.0], C=3)
    with pytest.raises(ValueError, match="proposal"):
        proposal_cum(np.array([2 ** 31, 2 ** 31]))


def test_one_weighted_draw_in_python_integers_and_the_plain_draw_is_unchanged():
    from sparsepoly_amd.pairwise import draw_candidates, draw_u64, proposal_cum, quantise_proposal

    q = quantise_proposal([0.0, 1.0, 2.0, 0.0, 5.5, 0.0])
    cum = proposal_cum(q)
    u = draw_u64(5, 2, 9, np.arange(200, dtype=np.uint64))
    got = draw_candidates(u, 6, cum)
    W = int(cum[-1])
    for ui, g in zip(u, got):
        x = ((int(ui) >> 32) * W) >> 32
        assert 0 <= x < W
        want = min(c for c in range(6) if int(cum[c]) > x)
        assert want == int(g)
    assert set(got) <= {1, 2, 4} and len(set(got)) == 3
    # without a table: the formula of DESIGN.md 19a, as before
    for C in (1, 2, 25, 20000, 2 ** 31 - 1):
        want = [((int(ui) >> 32) * C) >> 32 for ui in u]
        np.testing.assert_array_equal(draw_candidates(u, C), want)
        np.testing.assert_array_equal(draw_candidates(u, C, None), want)
    with pytest.raises(ValueError, match="cum must have shape"):
        draw_candidates(u, 5, cum)


def test_weighted_draws_follow_the_quantised_probabilities():
    """20 000 draws against q / sum(q) by the chi-square test and quantile of the uniform
    sampler's host test; a zero-weight candidate is never drawn"""
    from scipy.stats import chi2

    from sparsepoly_amd.pairwise import draw_candidates, draw_u64, proposal_cum, quantise_proposal

    w = (np.arange(N_CAND) + 1.0) ** 0.75
    w[[3, 11, 24]] = 0.0
    q = quantise_proposal(w)
    n = 20000
    c = draw_candidates(draw_u64(20261020, 0, np.arange(n, dtype=np.uint64), 0), N_CAND,
                        proposal_cum(q))
    counts = np.bincount(c, minlength=N_CAND)
    assert (counts[[3, 11, 24]] == 0).all()
    on = q > 0
    expect = n * q[on] / q.sum()
    stat = ((counts[on] - expect) ** 2 / expect).sum()
    print("chi-square over the %d weighted candidates: %.2f" % (on.sum(), stat))
    assert stat < chi2.ppf(1 - 1e-6, on.sum() - 1)
    # ... and it is not the uniform distribution
    flat = ((counts[on] - n / on.sum()) ** 2 / (n / on.sum())).sum()
    assert flat > chi2.ppf(1 - 1e-6, on.sum() - 1)


def test_restate_sample_with_a_table_draws_from_it():
    from sparsepoly_amd.pairwise import proposal_cum, quantise_proposal, restate_sample

    X, Z, _ = pair_problem()
    case = CASES[0]
    P, w, lams = _draw_params(case, 1 + case["k"] + 7 * case["degree"])
    I, E = sample_interactions()
    w_c = np.ones(N_CAND)
    w_c[[1, 4, 9, 16]] = 0.0
    cum = proposal_cum(quantise_proposal(w_c))
    t, _, _ = restate_sample(P, w, lams, X, Z, I, 2, 3, 1, 64, 99, 4, exclude=E, cum=cum)
    t0, _, _ = restate_sample(P, w, lams, X, Z, I, 2, 3, 1, 64, 99, 4, exclude=E)
    assert not np.array_equal(t, t0)
    assert not forbidden_dense(I, E)[t[:, 0], t[:, 2]].any()
    drawn = ~np.isin(t[:, 2], [1, 4, 9, 16])
    assert drawn.mean() > 0.9 and np.isin(t0[:, 2], [1, 4, 9, 16]).any()
    # max_draws = 1: the walk upwards may end on a candidate of weight 0 -- allowed, and it does
    t1, _, _ = restate_sample(P, w, lams, X, Z, I, 2, 3, 1, 1, 99, 4, exclude=E, cum=cum)
    assert np.isin(t1[:, 2], [1, 4, 9, 16]).any()
    assert (t1[t1[:, 0] == FULL_CTX, 2] == FREE_CAND).all()


# ---------------------------------------------------------------- 3. restate_warp
def test_restate_warp_against_its_definition():
    from sparsepoly_amd.pairwise import draw_candidates, draw_u64, restate_warp

    case = CASES[1]
    X, Z, _ = pair_problem()
    P, w, lams, margin = warp_params(case)
    I, E = sample_interactions()
    F = forbidden_dense(I, E)
    S = dense_scores(P, w, lams, X, Z, case["degree"])
    rows = np.repeat(np.arange(N_CTX), np.diff(I.indptr))
    posw = 0.25 + np.arange(I.nnz) % 5
    for n_neg, M, max_draws, mg in ((1, 8, 512, margin), (1, 8, 512, 0.0), (3, 33, 2112, margin),
                                    (1, 3, 192, margin), (1, 1, 1, 0.0), (3, 8, 8, margin)):
        t, sc, wt, tr, near, det = restate_warp(P, w, lams, X, Z, I, case["degree"], n_neg, M,
                                                max_draws, mg, 77, 3, exclude=E,
                                                positive_weights=posw, details=True)
        m = I.nnz * n_neg
        assert t.shape == (m, 3) and t.dtype == np.int32 and tr.dtype == np.int32
        np.testing.assert_array_equal(t[:, 0], np.repeat(rows, n_neg))
        np.testing.assert_array_equal(t[:, 1], np.repeat(I.indices, n_neg))
        assert not F[t[:, 0], t[:, 2]].any()
        for r in range(m):
            b, cp = t[r, 0], t[r, 1]
            thr = S[b, cp] - np.longdouble(mg)
            # the sequential definition, spelt out from the draws
            cand = draw_candidates(draw_u64(77, 3, r, np.arange(max_draws, dtype=np.uint64)),
                                   N_CAND)
            adm = [int(c) for c in cand if not F[b, c]][:M]
            N = next((i + 1 for i, c in enumerate(adm) if S[b, c] > thr), 0)
            if abs(float(near[r])) < 1e-12:
                continue   # (an exact tie with the threshold: longdouble may see it differently)
            assert tr[r] == N
            if N:
                assert t[r, 2] == adm[N - 1]
                A_b = N_CAND - F[b].sum()
                want = posw[r // n_neg] * np.log(max(1, A_b // N))
                assert abs(wt[r] - want) <= 1e-15 * max(1.0, want)
                assert near[r] == pytest.approx(
                    float(np.abs(S[b, adm[:N]] - thr).min()), abs=1e-12)
            elif adm:
                assert wt[r] == 0.0
                best = max(S[b, c] for c in adm)
                assert abs(float(S[b, t[r, 2]] - best)) < 1e-12
                first = next(c for c in adm if abs(float(S[b, c] - best)) < 1e-12)
                assert t[r, 2] == first or abs(float(S[b, first] - S[b, t[r, 2]])) == 0.0
            else:   # the fallback walk
                assert wt[r] == 0.0 and np.isinf(near[r]) and det[r][0].size == 0
                c = int(cand[-1])
                while True:
                    c = 0 if c + 1 == N_CAND else c + 1
                    if not F[b, c]:
                        break
                assert t[r, 2] == c
            assert abs(float(sc[r] - S[b, t[r, 2]])) < 1e-12
        if max_draws == 1:   # most triples take the walk
            assert (np.isinf(near)).mean() > 0.2 and (tr[np.isinf(near)] == 0).all()
        if mg == margin and M >= 8 and max_draws > 8:
            assert (tr == 0).any() and (tr == 1).any() and (tr > 4).any()
            assert (wt[tr > 0] >= 0).all() and (wt[(tr == 1)] > 0).any()
    # independent streams for n_negatives = 3; order permutes the slots only
    t, sc, wt, tr, near = restate_warp(P, w, lams, X, Z, I, case["degree"], 3, 8, 512, margin, 1,
                                       0, exclude=E, positive_weights=posw)
    free = np.repeat(N_CAND - F.sum(axis=1), np.diff(I.indptr))
    wide = free > 12
    assert ((t[0::3, 2] != t[1::3, 2]) | (t[0::3, 2] != t[2::3, 2]))[wide].mean() > 0.5
    assert (tr[0::3] != tr[1::3]).any()
    order = np.random.RandomState(0).permutation(len(t))
    out = restate_warp(P, w, lams, X, Z, I, case["degree"], 3, 8, 512, margin, 1, 0, exclude=E,
                       positive_weights=posw, order=order)
    for a, b in zip(out, (t, sc, wt, tr, near)):
        np.testing.assert_array_equal(a[order], b)
    # seed, epoch and the margin matter
    for kw in (dict(seed=2, epoch=0, margin=margin), dict(seed=1, epoch=1, margin=margin),
               dict(seed=1, epoch=0, margin=0.0)):
        other = restate_warp(P, w, lams, X, Z, I, case["degree"], 3, 8, 512, exclude=E, **kw)
        assert not np.array_equal(other[3], tr)
    with pytest.raises(ValueError, match="max_trials"):
        restate_warp(P, w, lams, X, Z, I, case["degree"], 1, 9, 8, 0.0, 1, 0)


# ---------------------------------------------------------------- 4. argument errors
def test_new_keyword_errors_come_before_any_handle(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker as R
    from sparsepoly_amd import engine, pairwise

    def boom(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", boom)
    monkeypatch.setattr(pairwise._BaseSparseFactorizationMachine, "_new_engine", boom)
    X, Z, t = pair_problem()
    I, E = sample_interactions()
    assert "warp" in pairwise.SAMPLERS
    for objective in ("list", "softmax"):
        with pytest.raises(ValueError, match="objective='pairwise'"):
            R().fit(X, Z, interactions=I, sampler="warp", objective=objective)
        with pytest.raises(ValueError, match="objective='pairwise'"):
            R().fit(X, Z, interactions=I, sampler="uniform", objective=objective,
                    sample_weight=np.ones(I.nnz))
    with pytest.raises(ValueError, match="not to sampler='host'"):
        R().fit(X, Z, interactions=I, proposal="popularity")
    with pytest.raises(ValueError, match="not to sampler='host'"):
        R().fit(X, Z, triples=t, proposal=np.ones(N_CAND))
    with pytest.raises(ValueError, match="give interactions, not triples"):
        R().fit(X, Z, triples=t, sampler="warp")
    with pytest.raises(ValueError, match="margin must be finite"):
        R().fit(X, Z, interactions=I, sampler="warp", margin=np.inf)
    with pytest.raises(ValueError, match="n_candidates"):
        R().fit(X, Z, interactions=I, sampler="warp", n_candidates=0)
    for sampler in ("uniform", "dynamic", "warp"):
        for bad in (-np.ones(N_CAND), np.full(N_CAND, np.nan), np.ones(N_CAND - 1),
                    np.zeros(N_CAND), "nope"):
            with pytest.raises(ValueError, match="proposal"):
                R().fit(X, Z, interactions=I, sampler=sampler, proposal=bad)
        for bad in (-np.ones(I.nnz), np.full(I.nnz, np.inf), np.ones(I.nnz + 1), "nope"):
            with pytest.raises(ValueError, match="sample_weight"):
                R().fit(X, Z, interactions=I, sampler=sampler, sample_weight=bad)
    for bad in (-np.ones(len(t)), np.ones(len(t) - 1), np.full(len(t), np.nan)):
        with pytest.raises(ValueError, match="sample_weight"):
            R().fit(X, Z, triples=t, sample_weight=bad)
    with pytest.raises(ValueError, match="sample_weight"):
        R().fit(X, Z, interactions=I, sample_weight=-np.ones(I.nnz))


def test_epoch_triples_with_weights_keeps_the_draws():
    from sklearn.utils import check_random_state

    from sparsepoly_amd.pairwise import epoch_triples

    I, E = sample_interactions()
    wq = 0.5 + np.arange(I.nnz) % 3
    plain = list(epoch_triples(check_random_state(5), 3, I, None, 2, True, True, E))
    pairs = list(epoch_triples(check_random_state(5), 3, I, None, 2, True, True, E, weights=wq))
    for a, (b, wt) in zip(plain, pairs):
        np.testing.assert_array_equal(a, b)
        assert wt.shape == (2 * I.nnz,)
        # every triple carries the weight of its positive
        key = {(r, c): v for r, c, v in zip(np.repeat(np.arange(N_CTX), np.diff(I.indptr)),
                                            I.indices, wq)}
        np.testing.assert_array_equal(wt, [key[(r, c)] for r, c, _ in b])


# ---------------------------------------------------------------- 5. prototypes
def test_header_capi_and_library_agree_on_the_new_symbols():
    import ctypes as C

    from sparsepoly_amd import _capi

    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"spfm_handle": C.c_void_p, "int": C.c_int, "double": C.c_double,
             "int64_t": C.c_int64, "const int32_t*": _capi._ip, "int32_t*": _capi._ip,
             "const int64_t*": _capi._lp, "int64_t*": _capi._lp, "double*": _capi._dp,
             "const double*": _capi._dp, "const uint32_t*": C.POINTER(C.c_uint32)}
    lib = _capi.load()
    for name in ("spfm_psgd_pairs_epoch_weighted", "spfm_psgd_pairs_set_proposal",
                 "spfm_psgd_pairs_set_positive_weights", "spfm_psgd_pairs_sample_warp"):
        m = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        types = [ctype[re.sub(r"\s*\w+$", "", a).replace(" *", "*")] for a in args]
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == types, name


# ---------------------------------------------------------------- 6. coverage and the cap
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_warp_cases_cover_every_trial_class_under_the_near_tie_cap(case):
    """At the parameters and margins the device tests use (margin 0 and the case's spread
    margin; n_candidates 3 / 8 / 33): the restated trials include N = 1, 1 < N <= 4 (inside the
    first batch of four), N > 4, N > 16 at 33 trials, and 0 (no violator); at most 5 % of a list
    has a tried candidate within 1e-6 of its threshold, and those triples belong to context 0
    (no entries: its scores are functions of the candidate alone and the quantised w ties
    them).  A case that missed either was reseeded by the rule of the list tests."""
    X, Z, _ = pair_problem()
    P, w, lams, margin, seed = _warp_case(CASES.index(case))
    print("seed %d (first: %d), spread margin %.6f"
          % (seed, 1 + case["k"] + 7 * case["degree"], margin))
    assert margin < 0.0
    for mg in (0.0, margin):
        seen, worst, outside = _coverage(P, w, lams, X, Z, case["degree"], (mg,))
        print("margin %.6f: classes %s, worst near-tie share %.4f" % (mg, sorted(seen), worst))
        assert worst <= NEAR_TIE_SHARE and outside == 0
    seen, _, _ = _coverage(P, w, lams, X, Z, case["degree"], (0.0, margin))
    assert seen == ALL_CLASSES
