"""``spfm_rank_*`` and what ``sparsepoly_amd.ranking`` builds on them, on the device.  Needs a real
MI355X: ``pytest -m gpu``.

Values are compared with the NumPy restatement (``restate_scores``) or with the NumPy towers of
``tests/test_ranking_host.py`` (``decomposed``; that file holds the two equal), evaluated in
``np.longdouble``.  The bound comes from the arithmetic and from no device run.  A score is a sum
of signed monomials in the entries of P, w, x and z.  Whatever the order of the additions, a
monomial goes through at most

    N = 2 (n_x + n_z) + 2 M + R' + 12

roundings: one per factor ``p x`` and one per DP addition in the two towers (``n_x``, ``n_z`` the
largest number of stored entries of a context / candidate row, dummy columns included; ``M`` the
degree, 0 for all-subsets), one per step of the product chain over the ``R'`` padded tower columns,
and 12 for the lane sums of the constants, the linear term and the closing
``+ (rowconst + colconst)``.  So ``|device - exact| <= (N + 2) 2^-53 S_abs`` per entry, where
``S_abs`` is the score of the model with every parameter and every input replaced by its magnitude
and all signs +1 (the sum of the magnitudes of the entry's monomials) and the 2 covers the
``longdouble`` reference (2^-11 of the bound).  Each case prints its largest error as a fraction
of its bound before asserting.

Orders are exact.  Where the device order is compared with the order of NumPy's own scores, the
NumPy side first asserts, before the device is touched, that the top K + 1 scores of every row are
at least ``CLEAR * max|score|`` apart; the seeds pass that on the CPU and no case is skipped.
"""
import ctypes
import itertools
import pickle

import numpy as np
import pytest
import scipy.sparse as sp
from test_ranking_host import abs_model, all_subsets, decomposed, fm, sides

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CLEAR = 1e-9


def _bound(est, X, Z, k_pad_cols):
    """(N + 2) 2^-53 S_abs per entry"""
    from sparsepoly_amd.ranking import _prepare

    Xa, Za = _prepare(est, X, Z)
    n_x = int(np.diff(Xa.indptr).max(initial=0))
    n_z = int(np.diff(Za.indptr).max(initial=0))
    M = max(est._obj_pred_args()[0], 0)
    N = 2 * (n_x + n_z) + 2 * M + k_pad_cols + 12
    S = decomposed(abs_model(est), abs(sp.csr_matrix(X)), abs(sp.csr_matrix(Z)), np.longdouble)
    return (N + 2) * U * S


def _padded_cols(est):
    degree, _, lower = est._obj_pred_args()
    k = est.lams_.shape[0]
    R = (k if degree == -1 else k * (degree - 1)) + (k if lower else 0)
    return (R + 3) // 4 * 4


def _check_values(got, want, bound, what):
    assert want.dtype == np.longdouble and got.shape == want.shape
    err = np.abs(got.astype(np.longdouble) - want)
    ok = bound > 0
    frac = float((err[ok] / bound[ok]).max(initial=0.0))
    print("%s: largest error %.3g of its bound" % (what, frac))
    assert (err <= bound).all(), (what, frac)


def _numpy_order(D, K):
    """(score descending, candidate ascending)"""
    return np.argsort(-D, axis=1, kind="stable")[:, :min(K, D.shape[1])].astype(np.int32)


def _clear(S, K):
    """the top K + 1 scores of every row are CLEAR * max|S| apart"""
    top = -np.sort(-S, axis=1)[:, :K + 1]
    if top.shape[1] > 1:
        assert np.diff(-top, axis=1).min() > CLEAR * np.abs(S).max(), "top K + 1 scores too close"


# ---------------------------------------------------------------- 1. values
def _estimators():
    from sparsepoly_amd import (SparseAllSubsetsClassifier, SparseAllSubsetsRegressor,
                                SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)

    cases = []
    for cls in (SparseFactorizationMachineRegressor, SparseFactorizationMachineClassifier):
        for degree, fl, lin in itertools.product((2, 3, 4, 5, 6), ("explicit", "augment", None),
                                                 (True, False)):
            cases.append(pytest.param(("fm", cls, degree, fl, lin),
                                      id="%s-%d-%s-%d" % (cls.__name__[-9:], degree, fl, lin)))
    for cls in (SparseAllSubsetsRegressor, SparseAllSubsetsClassifier):
        cases.append(pytest.param(("as", cls), id=cls.__name__))
    return cases


@pytest.mark.parametrize("spec", _estimators())
def test_scores_equal_the_restatement(spec):
    from sparsepoly_amd.ranking import restate_scores

    if spec[0] == "fm":
        _, cls, degree, fl, lin = spec
        est = fm(degree, 5, 12, fl, lin, seed=degree, cls=cls)  # random +-1 lams
    else:
        est = all_subsets(5, 12, seed=3, cls=spec[1])
    X, Z = sides(9, 70, 12, seed=7)
    want = restate_scores(est, X, Z, wide=True)
    bound = _bound(est, X, Z, _padded_cols(est))
    got = est.candidate_scores(X, Z)
    assert got.dtype == np.float64
    _check_values(got, want, bound, "scores %s" % (spec[1:],))
    idx, val = est.top_candidates(X, Z, 7)
    assert idx.dtype == np.int32 and idx.shape == val.shape == (9, 7)
    assert (val == np.take_along_axis(got, idx.astype(np.int64), axis=1)).all()
    assert (idx == _numpy_order(got, 7)).all()


# ---------------------------------------------------------------- 2. shapes
BS, CS, KS = (1, 63, 64, 65, 130), (1, 63, 65, 129, 1000), (1, 5, 30, 33)


def _shape_case(B, C, k, degree, z_entries, seed):
    """degree 3 explicit: R = 3k (k = 30: three chunks; k = 33: 99 -> 100); degree 2: R = k
    (k = 30: not a multiple of 4, k = 33: just past a chunk)"""
    est = fm(degree, k, 40, "explicit", True, seed=seed)
    X, Z = sides(B, C, 40, seed=seed, z_entries=z_entries, split=12)
    want = decomposed(est, X, Z, np.longdouble)
    bound = _bound(est, X, Z, _padded_cols(est))
    with est.ranker(Z) as r:
        D = r.scores(X)
        _check_values(D, want, bound, "B=%d C=%d k=%d degree=%d" % (B, C, k, degree))
        for K in (1, 7, C, C + 5):
            if K > 128:
                continue
            idx, val = r.top_k(X, K)
            assert idx.shape == val.shape == (B, min(K, C))
            assert (idx == _numpy_order(D, K)).all(), K
            assert (val == np.take_along_axis(D, idx.astype(np.int64), axis=1)).all(), K


@pytest.mark.parametrize("iB,iC", list(itertools.product(range(5), range(5))))
def test_shapes_rows_and_candidates(iB, iC):
    """every B x C, empty first rows on both sides (more than one row), candidates with one
    entry and with several, k and the degree cycling through the grid"""
    _shape_case(BS[iB], CS[iC], KS[(iB + iC) % 4], 2 + (iB + 2 * iC) % 2, 1 + (iB + iC) % 3,
                seed=10 * iB + iC)


@pytest.mark.parametrize("k,degree", list(itertools.product(KS, (2, 3))))
def test_shapes_components(k, degree):
    _shape_case(65, 129, k, degree, 2, seed=k)


# ---------------------------------------------------------------- 3. exact order
@pytest.mark.parametrize("kind", ["deg2", "deg3", "all-subsets"])
def test_exact_order_with_many_ties(kind):
    """small integers everywhere: every score is exact, ties are many, so idx pins the operand
    map of the matrix instruction and the tie rule -- also across strips and slabs"""
    rng = np.random.RandomState(5)
    d, k, B, C = 16, 5, 70, 300
    if kind == "all-subsets":
        est = all_subsets(k, d)
    else:
        est = fm(int(kind[3:]), k, d, "explicit", True)
        est.w_ = rng.randint(-2, 3, size=d).astype(float)
    est.P_ = rng.randint(-1, 3, size=est.P_.shape).astype(float)
    X = np.zeros((B, d))
    Z = np.zeros((C, d))
    for b in range(B):
        X[b, rng.choice(8, size=2, replace=False)] = rng.choice([-1.0, 1.0, 2.0], size=2)
    for c in range(C):
        Z[c, 8 + rng.choice(8, size=2, replace=False)] = rng.choice([-1.0, 1.0, 2.0], size=2)
    X, Z = sp.csr_matrix(X), sp.csr_matrix(Z)
    S = decomposed(est, X, Z)
    assert (S == np.round(S)).all() and np.abs(S).max() < 2 ** 40
    ties = sum(len(row) - len(np.unique(row)) for row in S)
    assert ties > B * C // 2
    for opts in ({}, {"cand_strip": 64, "row_slab": 64}):
        with est.ranker(Z) as r:
            r._engine.rank_set_partition(**opts)
            assert (r.scores(X) == S).all()
            for K in (1, 10, 128):
                idx, val = r.top_k(X, K)
                assert (idx == _numpy_order(S, K)).all(), (kind, opts, K)
                assert (val == np.take_along_axis(S, idx.astype(np.int64), axis=1)).all()


# ---------------------------------------------------------------- 4. one set of bits
def test_one_set_of_bits_under_every_partition():
    est = fm(3, 30, 40, "explicit", True, seed=2)
    X, Z = sides(130, 1000, 40, seed=2, split=12)
    ref = None
    with est.ranker(Z) as r:
        for slab, strip, rep in itertools.product((64, 128, 0), (64, 192, 0), (0, 1)):
            if rep and (slab, strip) != (0, 0):
                continue  # the second run: default partition
            r._engine.rank_set_partition(slab, strip)
            D = r.scores(X)
            tops = [r.top_k(X, K) for K in (7, 128)]
            if ref is None:
                ref = (D, tops)
                for K, (idx, val) in zip((7, 128), tops):
                    assert (idx == _numpy_order(D, K)).all()
                    assert (val == np.take_along_axis(D, idx.astype(np.int64), axis=1)).all()
            assert (D.view(np.int64) == ref[0].view(np.int64)).all(), (slab, strip)
            for (idx, val), (ridx, rval) in zip(tops, ref[1]):
                assert (idx == ridx).all(), (slab, strip)
                assert (val.view(np.int64) == rval.view(np.int64)).all(), (slab, strip)


# ---------------------------------------------------------------- 5. order on random data
@pytest.mark.parametrize("degree,seed", [(2, 11), (3, 12), (-1, 13)])
def test_order_on_random_data(degree, seed):
    from sparsepoly_amd.ranking import restate_scores

    est = all_subsets(6, 20, seed=seed) if degree == -1 else fm(degree, 6, 20, "explicit", True,
                                                                seed=seed)
    X, Z = sides(20, 200, 20, seed=seed)
    K = 10
    S = restate_scores(est, X, Z)
    _clear(S[1:], K)  # (row 0 is empty: its scores are the candidates' own, compared below too)
    _clear(S[:1], K)
    want = _numpy_order(S, K)
    idx, val = est.top_candidates(X, Z, K)
    assert (idx == want).all()
    bound = _bound(est, X, Z, _padded_cols(est))
    _check_values(val, np.take_along_axis(restate_scores(est, X, Z, wide=True),
                                          want.astype(np.int64), axis=1),
                  np.take_along_axis(bound, want.astype(np.int64), axis=1), "top-10 values")


# ---------------------------------------------------------------- 6. nothing of size B x C
def test_large_catalogue_stays_bounded():
    """B = 4096 contexts, C = 200 000 one-feature candidates, k = 30: the dense result would be
    6.5 GB; scratch and the drop of free device memory stay under 1 GiB"""
    from sparsepoly_amd.engine import HipEngine

    rng = np.random.RandomState(21)
    B, C, k, dc, K = 4096, 200_000, 30, 50, 10
    d = dc + C
    est = fm(2, k, d, None, True, seed=21)
    rows = np.repeat(np.arange(B), 3)
    cols = np.stack([rng.choice(dc, size=3, replace=False) for _ in range(B)]).ravel()
    X = sp.csr_matrix((rng.randn(3 * B), (rows, cols)), shape=(B, d))
    zval = 0.5 + rng.rand(C)
    Z = sp.csr_matrix((zval, (np.arange(C), dc + np.arange(C))), shape=(C, d))
    # NumPy towers of 64 sampled rows (degree 2): U = lams * (P x), V = P[:, item] z; the order
    # from the float64 scores, the values of the K entries in question in longdouble
    pick = np.sort(rng.choice(B, size=64, replace=False))
    P, w, lams = est.P_[0], est.w_, est.lams_
    Xs = X[pick].toarray()[:, :dc]
    Pc, Pz = P[:, :dc], P[:, dc:] * zval
    a1 = Xs @ Pc.T
    a2 = (a1 ** 2 - (Xs ** 2) @ (Pc ** 2).T) / 2
    S64 = (Xs @ w[:dc] + (a2 * lams).sum(axis=1))[:, None] + (w[dc:] * zval)[None, :] \
        + (a1 * lams) @ Pz
    _clear(S64, K)
    want = _numpy_order(S64, K)
    L = np.longdouble
    a1w = Xs.astype(L) @ Pc.T.astype(L)
    a2w = (a1w ** 2 - (Xs.astype(L) ** 2) @ (Pc.T.astype(L) ** 2)) / 2
    rowc = Xs.astype(L) @ w[:dc].astype(L) + (a2w * lams).sum(axis=1)
    aa1 = np.abs(Xs) @ np.abs(Pc).T
    aa2 = (aa1 ** 2 - (Xs ** 2) @ (Pc ** 2).T) / 2
    S = np.zeros(want.shape, dtype=L)
    Sabs = np.zeros(want.shape)
    for i in range(64):
        pz = P[:, dc + want[i]].astype(L) * zval[want[i]].astype(L)  # (k, K)
        S[i] = rowc[i] + w[dc + want[i]].astype(L) * zval[want[i]].astype(L) + (a1w[i] * lams) @ pz
        Sabs[i] = np.abs(Xs[i]) @ np.abs(w[:dc]) + aa2[i].sum() \
            + np.abs(w[dc + want[i]] * zval[want[i]]) + aa1[i] @ np.abs(pz.astype(np.float64))
    bound = (2 * (3 + 1) + 2 * 2 + 32 + 12 + 2) * U * Sabs * (1 + 1e-12)

    probe = HipEngine(0, "f64")
    free0 = probe.get_option("free_mem_mib")
    with est.ranker(Z) as r:
        idx, val = r.top_k(X, K)
        scratch = r._engine.rank_info()["scratch_kib"]
        free1 = r._engine.get_option("free_mem_mib")
    probe.close()
    print("scratch %d KiB, free memory %d -> %d MiB" % (scratch, free0, free1))
    assert 0 < scratch < 1024 * 1024 and free0 - free1 < 1024
    assert idx.shape == (B, K)
    assert (idx[pick] == want).all()
    _check_values(val[pick], S, bound.astype(np.longdouble), "sampled rows")


# ---------------------------------------------------------------- 7. errors
def test_errors():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    est = fm(2, 3, 10)
    X, Z = sides(4, 6, 10)
    r = est.ranker(Z)
    with pytest.raises(ValueError, match="exceeds"):
        r.top_k(X, _capi.RANK_MAX_K + 1)
    with pytest.raises(ValueError, match="K must be"):
        r.top_k(X, 0)
    idx, val = r.top_k(X, _capi.RANK_MAX_K)  # the cap itself is served; C = 6 columns come back
    assert idx.shape == (4, 6)
    with pytest.raises(TypeError):
        pickle.dumps(r)
    # the C entry refuses a K above the cap on its own
    eng = r._engine
    Xr = sp.csr_matrix(X)
    ia, ja, da = _capi.i64(Xr.indptr), _capi.i32(Xr.indices), _capi.f64(Xr.data)
    ko = ctypes.c_int64()
    rc = eng._lib.spfm_rank_topk(eng._h, 4, ia[1], ja[1], da[1], _capi.RANK_MAX_K + 1,
                                 idx.ctypes.data_as(_capi._ip), val.ctypes.data_as(_capi._dp),
                                 ctypes.byref(ko))
    assert rc == _capi.SPFM_ERR_UNSUPPORTED
    r.close()
    for call in (lambda: r.scores(X), lambda: r.top_k(X, 1)):
        with pytest.raises(ValueError, match="closed"):
            call()
    r.close()  # twice is fine

    # the C-level overlap check, reached through HipEngine directly
    eng = HipEngine(0, "f64")
    eng.set_params(est.P_, est.w_, est.lams_)
    with pytest.raises(ValueError, match="rank_set_candidates first"):
        eng.rank_scores(X)
    eng.rank_set_candidates(Z, 2, True, False)
    Xo = X.tolil()
    Xo[2, 7] = 1.5
    assert 7 in Z.indices
    for call in (lambda: eng.rank_scores(Xo.tocsr()), lambda: eng.rank_topk(Xo.tocsr(), 2)):
        with pytest.raises(ValueError, match="column 7 has stored entries"):
            call()
    assert eng.rank_scores(X).shape == (4, 6)
    assert eng.rank_info()["scratch_kib"] > 0
    eng.rank_release()
    assert eng.rank_info()["scratch_kib"] == 0
    with pytest.raises(ValueError, match="rank_set_candidates first"):
        eng.rank_topk(X, 1)
    eng.rank_set_candidates(Z, 2, True, False)
    eng.set_params(est.P_, est.w_, est.lams_)  # new parameters: the towers are gone
    assert eng.rank_info()["scratch_kib"] == 0
    with pytest.raises(ValueError, match="rank_set_partition"):
        eng.rank_set_partition(-1, 0)
    eng.close()


def test_dense_scores_above_one_gib_are_refused():
    from sparsepoly_amd import _capi

    C, B, d0 = 70_000, 2000, 4
    est = all_subsets(2, d0 + C)
    Z = sp.csr_matrix((np.ones(C), (np.arange(C), d0 + np.arange(C))), shape=(C, d0 + C))
    X = sp.csr_matrix((np.ones(B), (np.arange(B), np.arange(B) % d0)), shape=(B, d0 + C))
    assert B * C * 8 > _capi.RANK_SCORES_MAX_BYTES
    with est.ranker(Z) as r:
        with pytest.raises(ValueError, match="exceed the budget"):
            r.scores(X)
        eng = r._engine  # ... and by the C entry on its own
        ia, ja, da = _capi.i64(X.indptr), _capi.i32(X.indices), _capi.f64(X.data)
        rc = eng._lib.spfm_rank_scores(eng._h, B, ia[1], ja[1], da[1], None)
        assert rc == _capi.SPFM_ERR_INVALID
        idx, _ = r.top_k(X[:3], 2)  # the handle still serves
        assert idx.shape == (3, 2)
