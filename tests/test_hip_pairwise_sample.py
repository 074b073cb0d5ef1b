"""Negatives of the pairwise fit drawn on the device against the NumPy
restatement ``restate_sample``.  Needs a real MI355X: ``pytest -m gpu``.  The problem and the
cases come from ``tests/test_pairwise_host.py``, the interactions and the near-tie cap from
``tests/test_pairwise_sample_host.py``.

The uniform sampler is integer arithmetic and is compared exactly.  The dynamic sampler's choice
is compared exactly wherever the restated best score leads every different candidate of the set by
``NEAR_TIE`` = 1e-6 (1e3 times the margin bar ``MARGIN_ATOL``); elsewhere the device may pick any
admitted candidate within 1e-6 of the best, and at most 5 % of a list may be such triples.  The
epochs are held to the project's psgd bars (tests/test_hip_pairwise.py)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from test_pairwise_host import (CASES, GAMMA, HYPER, MARGIN_ATOL, N_CAND, N_CTX, case_id,
                                pair_params, pair_problem)
from test_pairwise_sample_host import (FREE_CAND, FULL_CTX, M_VALUES, NEAR_TIE, NEAR_TIE_SHARE,
                                       forbidden_dense, sample_interactions)

pytestmark = pytest.mark.gpu

P_ATOL = {"f64": 1e-9, "f32": 5e-5}
SL_RTOL = {"f64": 1e-10, "f32": 1e-5}
SHIFT = np.array([0, N_CTX, N_CTX], dtype=np.int32)   # context / candidate numbering -> rows


def _engine(case, X, Z, params=None, sampler=True):
    from sparsepoly_amd.engine import HipEngine

    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    P0, w0, lams = pair_params(case) if params is None else params
    eng = HipEngine(0, case["precision"])
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", case["loss"], case["reg"], case["degree"])
    if sampler:
        I, E = sample_interactions()
        eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I, I + E)
    return eng


def _hyper(case):
    return (case["degree"], HYPER["alpha"], HYPER["beta"], GAMMA[case["reg"]], HYPER["eta0"],
            HYPER["learning_rate"], HYPER["power_t"], case["batch"])


def check_dynamic(t_dev, sc_dev, P, w, lams, X, Z, degree, n_neg, M, max_draws, seed, epoch,
                  order=None):
    """the rule of the dynamic sampler's comparison; returns the share of near-tie triples and
    the share of triples whose negative is not their first admitted draw"""
    from sparsepoly_amd.pairwise import restate_sample

    I, E = sample_interactions()
    t, sc, gap, det = restate_sample(P, w, lams, X, Z, I, degree, n_neg, M, max_draws, seed,
                                     epoch, exclude=E, order=order, details=True)
    m = t.shape[0]
    slots = np.arange(m) if order is None else np.asarray(order)
    got = t_dev - SHIFT
    np.testing.assert_array_equal(got[:, :2], t[:, :2])
    clear = gap >= NEAR_TIE
    share = 1.0 - clear.mean()
    moved, worst = 0, 0.0
    for r, (adm, s_adm) in enumerate(det):
        c = got[slots[r], 2]
        assert c in adm, (r, c, adm)
        s_c = s_adm[list(adm).index(c)]
        assert s_c >= s_adm.max() - NEAR_TIE
        worst = max(worst, abs(float(sc_dev[slots[r]] - s_c)))
        moved += int(c != adm[0])
    print("m = %d, near-tie share %.4f, max |score - restated| = %.3e" % (m, share, worst))
    np.testing.assert_array_equal(got[clear, 2], t[clear, 2])
    assert worst <= MARGIN_ATOL
    assert share <= NEAR_TIE_SHARE
    return share, moved / m


# ------------------------------------------------------------------ 1. the uniform sampler
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("k_case", [0, 1, 2, 3], ids=["k5", "k30", "k40", "k70"])
def test_uniform_sampler_is_exact(k_case, precision):
    from sparsepoly_amd.pairwise import restate_sample

    case = dict(CASES[k_case], precision=precision)
    X, Z, _ = pair_problem()
    P, w, lams = pair_params(case)
    I, E = sample_interactions()
    F = forbidden_dense(I, E)
    eng = _engine(case, X, Z)
    try:
        for n_neg, max_draws, shuffled in ((1, 64, False), (3, 64, True), (3, 1, False),
                                           (1, 1, True)):
            m = I.nnz * n_neg
            order = np.random.RandomState(m).permutation(m) if shuffled else None
            got_m, t, sc = eng.psgd_pairs_sample(case["degree"], n_neg, 1, max_draws, 99, 4, order)
            want, _, _ = restate_sample(P, w, lams, X, Z, I, case["degree"], n_neg, 1, max_draws,
                                        99, 4, exclude=E, order=order)
            assert got_m == m and m % 16 != 0
            np.testing.assert_array_equal(t - SHIFT, want)
            assert (sc == 0).all()
            assert not F[t[:, 0], t[:, 2] - N_CTX].any()
            assert (t[t[:, 0] == FULL_CTX, 2] == N_CTX + FREE_CAND).all()
        after = eng.get_params()
        assert np.array_equal(after[0], P) and np.array_equal(after[1], w)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. the dynamic sampler
@pytest.mark.parametrize("M", M_VALUES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dynamic_sampler_against_the_restatement(case, M):
    X, Z, _ = pair_problem()
    P, w, lams = pair_params(case)
    n_neg = 3 if M == 3 else 1
    I, _ = sample_interactions()
    m = I.nnz * n_neg
    order = np.random.RandomState(M).permutation(m) if M == 8 else None
    eng = _engine(case, X, Z)
    try:
        _, t, sc = eng.psgd_pairs_sample(case["degree"], n_neg, M, 64 * M, 4242, 1, order)
    finally:
        eng.close()
    share, moved = check_dynamic(t, sc, P, w, lams, X, Z, case["degree"], n_neg, M, 64 * M, 4242,
                                 1, order)
    assert share <= n_neg / m     # context 0 alone, tests/test_pairwise_sample_host.py
    # the hardest of M is not the first admitted draw for a good part of the list: without this
    # the comparison above would show nothing about the scores
    assert moved > 0.3


# ------------------------------------------------------------------ 3. sampled epoch == uploaded
@pytest.mark.parametrize("case", [dict(CASES[1], batch=4), CASES[7]], ids=case_id)
def test_sampled_epoch_equals_uploaded_epoch(case):
    """batch = 4: 38 minibatches per epoch, one replayed run of 32 among them"""
    X, Z, _ = pair_problem()
    prec = case["precision"]
    a = _engine(case, X, Z)
    b = _engine(case, X, Z, sampler=False)
    try:
        it_a = it_b = 1
        for ep in range(2):
            m, t, _ = a.psgd_pairs_sample(case["degree"], 1, 8, 512, 7, ep)
            sl_a, it_a = a.psgd_pairs_epoch_sampled(*_hyper(case), case["fit_linear"], it_a)
            sl_b, it_b = b.psgd_pairs_epoch(*_hyper(case), t, case["fit_linear"], it_b)
            Pa, wa = a.get_params()
            Pb, wb = b.get_params()
            print("epoch %d: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
                  % (ep + 1, np.abs(Pa - Pb).max(), np.abs(wa - wb).max(),
                     abs(sl_a - sl_b) / abs(sl_b)))
            assert it_a == it_b == 1 + (ep + 1) * -(-m // case["batch"])
            np.testing.assert_allclose(sl_a, sl_b, rtol=SL_RTOL[prec])
            np.testing.assert_allclose(Pa, Pb, rtol=0, atol=P_ATOL[prec])
            np.testing.assert_allclose(wa, wb, rtol=0, atol=P_ATOL[prec])
        assert np.abs(Pa - pair_params(case)[0]).max() > 1e-4     # it did train
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 4. three epochs, teacher-forced
@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=case_id)
def test_three_epochs_without_compounding(case):
    """every epoch is compared from the parameters the device holds at its start: a flipped
    argmax can never be blamed on accumulated rounding"""
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z, _ = pair_problem()
    lams = pair_params(case)[2]
    prec = case["precision"]
    I, _ = sample_interactions()
    eng = _engine(case, X, Z)
    try:
        it = 1
        for ep in range(3):
            P, w = eng.get_params()
            order = np.random.RandomState(ep).permutation(I.nnz)
            m, t, sc = eng.psgd_pairs_sample(case["degree"], 1, 8, 512, 31, ep, order)
            check_dynamic(t, sc, P, w, lams, X, Z, case["degree"], 1, 8, 512, 31, ep, order)
            sl, it_new = eng.psgd_pairs_epoch_sampled(*_hyper(case), case["fit_linear"], it)
            Pr, wr, slr, itr = restate_pairwise_epoch(
                P, w, lams, X, Z, t - SHIFT, case["degree"], case["loss"], case["reg"],
                gamma=GAMMA[case["reg"]], batch_size=case["batch"],
                fit_linear=case["fit_linear"], it=it, **HYPER)
            Pd, wd = eng.get_params()
            assert it_new == itr
            np.testing.assert_allclose(sl, float(slr), rtol=SL_RTOL[prec])
            np.testing.assert_allclose(Pd, Pr, rtol=0, atol=P_ATOL[prec])
            np.testing.assert_allclose(wd, wr, rtol=0, atol=P_ATOL[prec])
            it = it_new
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. error codes
def test_error_codes_behind_the_c_abi():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    INV, OK = _capi.SPFM_ERR_INVALID, _capi.SPFM_OK
    case = CASES[0]
    X, Z, tr = pair_problem()
    I, E = sample_interactions()
    Fm = sp.csr_matrix(I + E)
    Fm.sort_indices()
    eng = _engine(case, X, Z, sampler=False)
    lib, h = eng._lib, eng._h

    def set_sampler(pos, forb=None, n_ctx=N_CTX, n_cand=N_CAND):
        pp = np.ascontiguousarray(pos.indptr, dtype=np.int64)
        pi = np.ascontiguousarray(pos.indices, dtype=np.int32)
        fp = fi = None
        if forb is not None:
            fp = np.ascontiguousarray(forb.indptr, dtype=np.int64)
            fi = np.ascontiguousarray(forb.indices, dtype=np.int32)
        return lib.spfm_psgd_pairs_set_sampler(
            h, n_ctx, n_cand, pp.ctypes.data_as(_capi._lp), pi.ctypes.data_as(_capi._ip),
            None if fp is None else fp.ctypes.data_as(_capi._lp),
            None if fi is None else fi.ctypes.data_as(_capi._ip))

    def sample(degree=2, n_neg=1, M=4, max_draws=64, order=None, handle=None):
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
        return lib.spfm_psgd_pairs_sample(handle or h, degree, n_neg, M, max_draws, 1, 0,
                                          None if o is None else o.ctypes.data_as(_capi._ip),
                                          None, None)

    def epoch_sampled(batch=8, it=1, lr=1, handle=None):
        itc, sl = C.c_int64(it), C.c_double()
        return lib.spfm_psgd_pairs_epoch_sampled(handle or h, 2, 0.01, 0.5, 0.003, 0.05, lr, 0.8,
                                                 batch, 1, C.byref(itc), C.byref(sl))

    before = eng.get_params()
    assert sample() == INV                   # no sampler set
    assert epoch_sampled() == INV            # nothing sampled
    # set_sampler: the shapes, the index lists, the supersets, a full row, shared columns
    assert set_sampler(I, Fm, n_ctx=N_CTX - 1) == INV
    unsorted = I.copy()
    r1 = slice(unsorted.indptr[1], unsorted.indptr[2])
    unsorted.indices[r1] = unsorted.indices[r1][::-1]
    assert set_sampler(unsorted, None) == INV
    assert set_sampler(I, unsorted) == INV
    outside = I.copy()
    outside.indices[-1] = N_CAND
    assert set_sampler(outside, None) == INV
    assert set_sampler(I, sp.csr_matrix(E)) == INV          # forbidden lacks the positives
    full = sp.lil_matrix(Fm)
    full[FULL_CTX, FREE_CAND] = 1.0
    full = sp.csr_matrix(full)
    full.sort_indices()
    assert set_sampler(I, full) == INV
    assert set_sampler(sp.csr_matrix((N_CTX, N_CAND)), None) == INV     # no positive
    assert sample() == INV                   # none of these left a sampler behind
    assert set_sampler(I, Fm) == OK
    # sample: its own arguments
    assert sample(degree=3) == INV
    assert sample(n_neg=0) == INV
    assert sample(M=0) == INV
    assert sample(max_draws=0) == INV
    assert sample(order=np.zeros(I.nnz)) == INV              # not a permutation
    assert epoch_sampled() == INV            # still nothing sampled
    assert sample() == OK
    assert epoch_sampled(batch=0) == INV
    assert epoch_sampled(it=0) == INV
    assert epoch_sampled(lr=4) == INV
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert epoch_sampled() == OK             # the same handle trains from the sampled list
    # a plain epoch uploads over the sampled list
    ts = (tr + SHIFT).astype(np.int32)
    eng.psgd_pairs_epoch(2, 0.01, 0.5, 0.003, 0.05, "optimal", 0.8, 8, ts, True, 1)
    before = eng.get_params()
    assert epoch_sampled() == INV
    assert sample() == OK
    eng.psgd_pairs_eval(2, True, ts)
    assert epoch_sampled() == INV
    with pytest.raises(ValueError, match="not the output"):
        eng.psgd_pairs_epoch_sampled(2, 0.01, 0.5, 0.003, 0.05, "optimal", 0.8, 8, True, 1)
    # new data drops the sampler
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.configure("psgd", case["loss"], case["reg"], case["degree"])
    assert sample() == INV
    with pytest.raises(ValueError, match="set_sampler first"):
        eng.psgd_pairs_sample(2, 1, 4, 64, 1, 0)
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    eng.close()
    # a column shared between a context with a positive and a candidate
    Xb = sp.lil_matrix(X)
    Xb[1, 80] = 1.0
    eng = _engine(case, sp.csr_matrix(Xb), Z, sampler=False)
    lib, h = eng._lib, eng._h
    before = eng.get_params()
    assert set_sampler(I, Fm) == INV
    with pytest.raises(ValueError, match="column 80"):
        eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I, Fm)
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    eng.close()
    # a handle configured for another solver
    P0, w0, lams = pair_params(case)
    eng = HipEngine(0, "f64")
    eng.set_data(S, np.zeros(S.shape[0]))
    eng.set_params(P0, w0, lams)
    eng.configure("pcd", "logistic", "l1", 2)
    lib, h = eng._lib, eng._h
    assert set_sampler(I, Fm) == OK
    assert sample() == INV
    assert epoch_sampled() == INV
    after = eng.get_params()
    assert np.array_equal(P0, after[0]) and np.array_equal(w0, after[1])
    eng.close()


# ------------------------------------------------------------------ 6. the estimator
E2E_EPOCHS = 3
E2E_KW = dict(degree=2, n_components=6, fit_lower=None, fit_linear=True, regularizer="l1",
              alpha=1e-3, beta=1e-2, gamma=1e-4, eta0=0.5, learning_rate="invscaling", power_t=0.3,
              batch_size=64, max_iter=E2E_EPOCHS, tol=-1.0, n_iter_no_change=1000, shuffle=True,
              random_state=3, precision="f64")


def planted_problem():
    """(X, Z, train, held): 200 contexts (a user id and two of eight attributes), 60 candidates
    (an item id); per context the four best candidates of a planted two-tower model are the
    training interactions, the next two are held out (the generator of
    tests/test_hip_pairwise.py)"""
    rng = np.random.RandomState(7)
    B, Cn, r = 200, 60, 4
    order = np.argsort(-(rng.randn(B, r) @ rng.randn(Cn, r).T), axis=1)
    train = sp.csr_matrix((np.ones(B * 4), (np.repeat(np.arange(B), 4), order[:, :4].ravel())),
                          shape=(B, Cn))
    held = sp.csr_matrix((np.ones(B * 2), (np.repeat(np.arange(B), 2), order[:, 4:6].ravel())),
                         shape=(B, Cn))
    d = B + 8 + Cn
    attr = np.stack([rng.choice(8, 2, replace=False) for _ in range(B)])
    X = sp.csr_matrix((np.ones(3 * B),
                       (np.repeat(np.arange(B), 3),
                        np.column_stack([np.arange(B), B + attr]).ravel())), shape=(B, d))
    Z = sp.csr_matrix((np.ones(Cn), (np.arange(Cn), B + 8 + np.arange(Cn))), shape=(Cn, d))
    return X, Z, train, held


def test_ranker_fit_with_the_dynamic_sampler():
    """the fit against the loop rebuilt from restate_sample + restate_pairwise_epoch under the
    same random_state, every epoch from the parameters a callback read off the device"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import restate_pairwise_epoch, restate_sample

    X, Z, train, held = planted_problem()
    d = X.shape[1]
    seen = []
    est = SparseFactorizationMachineRanker(
        callback=lambda e: seen.append((e.P_.copy(), e.w_.copy())), n_calls=1, **E2E_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=train, n_negatives=2, resample=True, sampler="dynamic",
                n_candidates=4, exclude=held)
    assert len(seen) == E2E_EPOCHS
    rng = check_random_state(E2E_KW["random_state"])
    P0 = 0.01 * rng.randn(1, 6, d)
    lams = np.ones(6)
    seed = rng.randint(0, 2 ** 31 - 1)
    m = train.nnz * 2
    starts = [(P0, np.zeros(d))] + seen[:-1]
    it = 1
    Fd = forbidden_dense(train, held)
    for ep, (P, w) in enumerate(starts):
        order = rng.permutation(m)
        t, _, gap = restate_sample(P, w, lams, X, Z, train, 2, 2, 4, 256, seed, ep, exclude=held,
                                   order=order)
        assert not Fd[t[:, 0], t[:, 2]].any()
        share = (gap < NEAR_TIE).mean()
        print("epoch %d: near-tie share %.4f" % (ep + 1, share))
        assert share <= NEAR_TIE_SHARE
        Pr, wr, _, it = restate_pairwise_epoch(P, w, lams, X, Z, t, 2, "logistic", "l1", 1e-3,
                                               1e-2, 1e-4, 0.5, "invscaling", 0.3, 64, True, it)
        # the epoch can only be compared if the device drew the restated list: its scores meet
        # MARGIN_ATOL, so a best score that leads by more than twice that fixes the choice
        assert gap.min() > 2 * MARGIN_ATOL, gap.min()
        np.testing.assert_allclose(seen[ep][0], Pr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(seen[ep][1], wr, rtol=0, atol=1e-9)
    assert est.it_ == it == 1 + E2E_EPOCHS * 25 and est.n_iter_ == E2E_EPOCHS - 1
    np.testing.assert_array_equal(est.P_, seen[-1][0])
    # sample_negatives on the fitted object
    tn, sn = est.sample_negatives(X, Z, train, n_negatives=2, n_candidates=4, exclude=held,
                                  random_state=5)
    want, swant, gap = restate_sample(est.P_, est.w_, est.lams_, X, Z, train, 2, 2, 4, 256,
                                      check_random_state(5).randint(0, 2 ** 31 - 1), 0,
                                      exclude=held)
    assert tn.shape == (m, 3) and not Fd[tn[:, 0], tn[:, 2]].any()
    clear = gap >= NEAR_TIE
    assert 1.0 - clear.mean() <= NEAR_TIE_SHARE
    np.testing.assert_array_equal(tn[:, :2], want[:, :2])
    np.testing.assert_array_equal(tn[clear], want[clear])
    np.testing.assert_allclose(sn[clear], swant[clear], rtol=0, atol=MARGIN_ATOL)


def test_host_sampler_keeps_its_bits_and_honours_exclude():
    """``sampler='host'`` is the route of a fit without the new keywords, bit for bit.  Bits can
    only be compared where the fit has them: the gradient scatter uses f64 atomics, so two runs
    of one fit with 64 triples per minibatch differ in the last bits (5e-17 here), on the parent
    commit too.  With one triple per minibatch no two atomics of a launch meet at an address
    (every candidate of this problem has a column of its own) and the fit is a function of its
    draws alone: that is compared bit for bit; the batch of 64 at the project's psgd bar."""
    from sparsepoly_amd import SparseFactorizationMachineRanker

    X, Z, train, held = planted_problem()
    fits = []
    for batch, max_iter in ((1, 2), (64, E2E_EPOCHS)):
        for kw in ({}, dict(sampler="host", n_candidates=4, exclude=None)):
            est = SparseFactorizationMachineRanker(**dict(E2E_KW, batch_size=batch,
                                                          max_iter=max_iter))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                est.fit(X, Z, interactions=train, n_negatives=2, resample=True, **kw)
            fits.append(est)
    assert np.array_equal(fits[0].P_, fits[1].P_) and np.array_equal(fits[0].w_, fits[1].w_)
    assert fits[0].it_ == fits[1].it_ == 1 + 2 * 1600
    print("batch 64: max|dP| = %.3e" % np.abs(fits[2].P_ - fits[3].P_).max())
    np.testing.assert_allclose(fits[2].P_, fits[3].P_, rtol=0, atol=1e-9)
    np.testing.assert_allclose(fits[2].w_, fits[3].w_, rtol=0, atol=1e-9)
    assert fits[2].it_ == fits[3].it_
    fits = fits[2:]
    # exclude reaches sample_triples: the draws, and with them the fit, change
    est = SparseFactorizationMachineRanker(**E2E_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=train, n_negatives=2, exclude=held)
    assert not np.array_equal(est.P_, fits[0].P_)
    # the uniform device sampler trains too
    est = SparseFactorizationMachineRanker(**E2E_KW)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, interactions=train, n_negatives=2, sampler="uniform", resample=False)
    assert est.it_ == 1 + E2E_EPOCHS * 25
    assert np.isfinite(est.P_).all() and np.abs(est.P_).max() > 0.011
