"""``spfm_rank_eval`` / ``spfm_rank_topk_excl`` and what ``sparsepoly_amd.ranking`` builds on them,
on the device.  Needs a real MI355X: ``pytest -m gpu``.

Every expectation is computed in NumPy from the dense ``ranker.scores(X)`` by the definition

    rank[b, t] = #{ c not in E_b, c != t : score[b, c] > score[b, t]
                                           or (score[b, c] == score[b, t] and c < t) }

and compared with ``==``: there is no tolerance anywhere.  The shapes come from the 64 x 64 tiles:
B = 70 is two row tiles, the second partial; C = 200 is four candidate tiles, the last partial;
k = 5 gives tower widths that are padded (5 -> 8, 10 -> 12).  Each estimator is run with the
default partition and with ``rank_set_partition(64, 64)`` -- two slabs, four strips -- and both
runs must give the NumPy answer.
"""
import types

import numpy as np
import pytest
import scipy.sparse as sp
from test_ranking_host import all_subsets, fm, sides

pytestmark = pytest.mark.gpu

B, C, D_FEAT, K_COMP = 70, 200, 16, 5
TIED = (3, 66, 130)  # three identical candidate rows, in three different tiles


def _lists():
    """targets and excluded candidates per context row (ascending, disjoint)"""
    rng = np.random.RandomState(42)
    T = [[] for _ in range(B)]
    E = [[] for _ in range(B)]
    T[1], E[1] = [0], [63, 64, 199]
    T[2] = [63, 64, 127, 128, 199]
    T[3] = sorted({0, 199} | set(rng.choice(np.arange(1, 199), size=62, replace=False).tolist()))
    E[3] = [c for c in range(C) if c not in T[3]]      # n_eff == |T_b|
    T[4] = [66]                                         # the middle one of the tied candidates
    T[5], E[5] = [3], [66]
    T[6], E[6] = [130], [0]
    T[7], E[7] = [0, 63, 128, 150, 199], list(range(64, 128))  # a whole strip of the 64-wide run
    T[8] = list(TIED)                                   # all three tied ones are targets
    T[65], E[65] = [1, 64, 100, 127, 198], [0, 63, 128, 199]
    T[69], E[69] = [199], [63, 64]
    for b in range(9, 64):
        nt, ne = rng.randint(0, 6), rng.randint(0, 51)
        pick = rng.choice(C, size=nt + ne, replace=False)
        T[b], E[b] = sorted(pick[:nt].tolist()), sorted(pick[nt:].tolist())
    assert len(T[0]) == 0 and len(T[3]) == 64 and all(len(t) <= 64 for t in T)
    return T, E


def _csr(rows, n_cand=C):
    r = np.array([b for b, cs in enumerate(rows) for _ in cs], dtype=np.int64)
    c = np.array([x for cs in rows for x in cs], dtype=np.int64)
    return sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(B, n_cand)).tocsr()


def _beats(v, c, s, t):
    return (v > s) | ((v == s) & (c < t))


def numpy_ranks(D, T, E):
    """ranks and scores in the order of the canonical pattern, n_eff per row"""
    ranks, scores, n_eff = [], [], []
    cols = np.arange(C)
    for b in range(B):
        ok = np.isfinite(D[b])
        ok[E[b]] = False
        n_eff.append(C - len(E[b]))
        for t in T[b]:
            scores.append(D[b, t])
            m = ok & (cols != t)
            ranks.append(int(_beats(D[b, m], cols[m], D[b, t], t).sum())
                         if np.isfinite(D[b, t]) else -1)
    return np.array(ranks, dtype=np.int32), np.array(scores), np.array(n_eff, dtype=np.int32)


def numpy_topk(D, E, K):
    """(value descending, index ascending) over the admissible candidates; -1 / NaN after them"""
    Ko = min(K, C)
    idx = np.full((B, Ko), -1, dtype=np.int32)
    val = np.full((B, Ko), np.nan)
    for b in range(B):
        ok = np.isfinite(D[b])
        ok[E[b]] = False
        cand = np.flatnonzero(ok)
        order = cand[np.argsort(-D[b, cand], kind="stable")][:Ko]
        idx[b, :len(order)] = order
        val[b, :len(order)] = D[b, order]
    return idx, val


def _same_lists(got, want):
    (gi, gv), (wi, wv) = got, want
    assert gi.dtype == np.int32 and gi.shape == wi.shape and gv.shape == wv.shape
    assert (gi == wi).all()
    pad = wi < 0
    assert np.isnan(gv[pad]).all()
    assert (gv[~pad].view(np.int64) == wv[~pad].view(np.int64)).all()


def _estimator(kind):
    if kind == "deg2-linear":
        return fm(2, K_COMP, D_FEAT, None, True, seed=1)
    if kind == "deg3-explicit":
        return fm(3, K_COMP, D_FEAT, "explicit", True, seed=2)
    if kind == "all-subsets":
        return all_subsets(K_COMP, D_FEAT, seed=3)
    est = fm(2, K_COMP, D_FEAT, None, True, seed=4)
    est.set_params(precision="f32")
    return est


@pytest.fixture(scope="module", params=["deg2-linear", "deg3-explicit", "all-subsets", "deg2-f32"])
def case(request):
    """one estimator with its ranker open, the dense scores and the NumPy answers (made once)"""
    est = _estimator(request.param)
    X, Z = sides(B, C, D_FEAT, seed=11)
    Z = Z.tolil()
    for c in TIED[1:]:
        Z[c] = Z[TIED[0]]
    Z = Z.tocsr()
    T, E = _lists()
    with est.ranker(Z) as r:
        D = r.scores(X)
        # the tie case is real: the three columns are equal, so the index rule decides
        assert (D[:, TIED[0]] == D[:, TIED[1]]).all() and (D[:, TIED[0]] == D[:, TIED[2]]).all()
        assert np.isfinite(D).all() and len(np.unique(D[4])) > C // 2
        ranks, scores, n_eff = numpy_ranks(D, T, E)
        yield types.SimpleNamespace(est=est, X=X, Z=Z, T=T, E=E, Tm=_csr(T), Em=_csr(E), r=r, D=D,
                                    ranks=ranks, scores=scores, n_eff=n_eff)


PARTITIONS = [(0, 0), (64, 64)]


@pytest.mark.parametrize("part", PARTITIONS)
def test_ranks_and_scores_equal_the_definition(case, part):
    c = case
    c.r._engine.rank_set_partition(*part)
    ranks, scores = c.r.ranks(c.X, c.Tm, c.Em)
    assert ranks.dtype == np.int32 and scores.dtype == np.float64
    assert (scores.view(np.int64) == c.scores.view(np.int64)).all()  # bit for bit
    assert (ranks == c.ranks).all()
    _, _, n_eff = c.r._engine.rank_eval(c.r._contexts(c.X), (c.Tm.indptr, c.Tm.indices),
                                        (c.Em.indptr, c.Em.indices))
    assert (n_eff == c.n_eff).all()
    # the tied candidates: 3 beats 66 beats 130 at one score
    tp = c.Tm.indptr
    s4 = c.D[4, 66]
    assert (c.D[4, :66] == s4).sum() >= 1  # candidate 3 at least
    assert ranks[tp[4]] == (c.D[4] > s4).sum() + (c.D[4, :66] == s4).sum()
    assert ranks[tp[8] + 1] == ranks[tp[8]] + 1 and ranks[tp[8] + 2] == ranks[tp[8]] + 2
    # n_eff == |T_b|: the ranks of the row are a permutation
    assert sorted(ranks[tp[3]:tp[4]]) == list(range(64))
    # without exclusions (eptr NULL: the other instantiation of the count pass)
    none = [[] for _ in range(B)]
    want, _, want_eff = numpy_ranks(c.D, c.T, none)
    got, gscores, got_eff = c.r._engine.rank_eval(c.r._contexts(c.X),
                                                  (c.Tm.indptr, c.Tm.indices))
    assert (got == want).all() and (got_eff == C).all() and (want_eff == C).all()
    assert (gscores.view(np.int64) == c.scores.view(np.int64)).all()
    c.r._engine.rank_set_partition(0, 0)


@pytest.mark.parametrize("part", PARTITIONS)
def test_top_k_with_exclusions(case, part):
    c = case
    c.r._engine.rank_set_partition(*part)
    none = [[] for _ in range(B)]
    for K in (1, 10, 128):
        _same_lists(c.r.top_k(c.X, K, exclude=c.Em), numpy_topk(c.D, c.E, K))
        plain = c.r.top_k(c.X, K)
        _same_lists(plain, numpy_topk(c.D, none, K))
        for same in (c.r.top_k(c.X, K, exclude=None),
                     c.r.top_k(c.X, K, exclude=sp.csr_matrix((B, C)))):
            assert (same[0] == plain[0]).all()
            assert (same[1].view(np.int64) == plain[1].view(np.int64)).all()
    idx, val = c.r.top_k(c.X, 128, exclude=c.Em)
    assert (idx[3, :64] >= 0).all() and (idx[3, 64:] == -1).all() and np.isnan(val[3, 64:]).all()
    assert sorted(idx[3, :64]) == c.T[3]
    c.r._engine.rank_set_partition(0, 0)


STRESS_C, STRESS_CTX = 400, 8  # candidates (seven tiles, the last partial); context columns
STRESS_KEPT = (0, 63, 64, 255, 399)  # all that row 5 keeps


@pytest.fixture(scope="module", params=["ascending", "descending"])
def stress(request):
    """Scores that are exact small integers and strictly monotone in the candidate id for every
    row: candidate c has the one entry 1 in a column of its own and the linear term carries
    +-(c + 1); P is zero on the candidate columns, so the product adds exact zeros.  Ascending,
    every candidate beats all before it: every one survives and every tile past the buffer's
    capacity forces a compaction.  Descending, nothing survives the first compaction."""
    rng = np.random.RandomState(7)
    up = request.param == "ascending"
    est = fm(2, 1, STRESS_CTX + STRESS_C, None, True, seed=5)
    est.P_[:] = 0.0
    est.P_[0, 0, :STRESS_CTX] = rng.randint(-1, 2, size=STRESS_CTX)
    est.w_[:STRESS_CTX] = rng.randint(-3, 4, size=STRESS_CTX)
    est.w_[STRESS_CTX:] = (1.0 if up else -1.0) * np.arange(1, STRESS_C + 1)
    X = sp.csr_matrix(np.hstack([rng.randint(-2, 3, size=(B, STRESS_CTX)).astype(np.float64),
                                 np.zeros((B, STRESS_C))]))
    Z = sp.csr_matrix(np.hstack([np.zeros((STRESS_C, STRESS_CTX)), np.eye(STRESS_C)]))
    # (a) every row leaves out about one candidate in seven, (b) some rows their entire
    # unexcluded top 130 as well, (c) row 5 all but five candidates
    top = range(STRESS_C - 130, STRESS_C) if up else range(130)
    E = [[c for c in range(STRESS_C) if (c + b) % 7 == 0] for b in range(B)]
    for b in (2, 33, 64, 69):
        E[b] = sorted(set(E[b]) | set(top))
    E[5] = [c for c in range(STRESS_C) if c not in STRESS_KEPT]
    with est.ranker(Z) as r:
        D = r.scores(X)
        assert D.shape == (B, STRESS_C) and (D == np.rint(D)).all() and np.abs(D).max() < 2 ** 20
        assert ((np.diff(D, axis=1) > 0) if up else (np.diff(D, axis=1) < 0)).all()
        yield types.SimpleNamespace(r=r, X=X, D=D, E=E, Em=_csr(E, STRESS_C))


@pytest.mark.parametrize("excluded", [False, True])
def test_selection_stress(stress, excluded):
    """The ranker's entry to the shared selection under forced compactions, with and without the
    exclusion masks; K = 128 fills the buffer to its capacity K + 64.  Default partition (one
    strip of seven tiles) and cand_strip = 128 (four lists to merge)."""
    s = stress
    E = s.E if excluded else [[] for _ in range(B)]
    for strip in (0, 128):
        s.r._engine.rank_set_partition(0, strip)
        for K in (1, 10, 128):
            got = s.r.top_k(s.X, K, exclude=s.Em) if excluded else s.r.top_k(s.X, K)
            _same_lists(got, numpy_topk(s.D, E, K))
            if excluded and K >= 10:  # the short list: five entries, then -1 / NaN
                assert sorted(got[0][5, :5]) == list(STRESS_KEPT) and (got[0][5, 5:] == -1).all()
                assert np.isnan(got[1][5, 5:]).all()
    s.r._engine.rank_set_partition(0, 0)


def test_evaluate_and_rank_metrics(case):
    from sparsepoly_amd.ranking import metrics_from_ranks

    c = case
    ks = (1, 10)
    want = metrics_from_ranks(c.Tm.indptr, c.ranks, c.n_eff, ks)
    assert want["n_rows_scored"] == sum(1 for t in c.T if t)
    np.testing.assert_equal(c.r.evaluate(c.X, c.Tm, c.Em, ks=ks), want)
    np.testing.assert_equal(c.est.rank_metrics(c.X, c.Z, c.Tm, c.Em, ks=ks), want)
    # unsorted input with duplicates is canonicalised first
    coo = c.Tm.tocoo()
    shuffled = sp.coo_matrix((np.ones(2 * coo.nnz), (np.tile(coo.row, 2)[::-1],
                                                     np.tile(coo.col, 2)[::-1])), shape=(B, C))
    np.testing.assert_equal(c.r.evaluate(c.X, shuffled, c.Em, ks=ks), want)
    with pytest.raises(ValueError, match="excluded"):
        c.r.evaluate(c.X, c.Tm, c.Tm)


def test_errors_through_the_c_abi_leave_the_outputs_alone():
    """the library's own checks, the Python checks bypassed"""
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    est = fm(2, 3, 10)
    X, Z = sides(4, 100, 10)
    Xr = sp.csr_matrix(X)
    ia, ja, da = _capi.i64(Xr.indptr), _capi.i32(Xr.indices), _capi.f64(Xr.data)
    eng = HipEngine(0, "f64")
    eng.set_params(est.P_, est.w_, est.lams_)

    def call(tptr, tidx, eptr=None, eidx=None):
        tp, ti = _capi.i64(tptr), _capi.i32(tidx)
        ep, ei = (_capi.i64(eptr), _capi.i32(eidx)) if eptr is not None else ((None, None),) * 2
        ranks = np.full(max(len(tidx), 1), -77, dtype=np.int32)
        scores = np.full(max(len(tidx), 1), -77.0)
        n_eff = np.full(4, -77, dtype=np.int32)
        rc = eng._lib.spfm_rank_eval(eng._h, 4, ia[1], ja[1], da[1], tp[1], ti[1], ep[1], ei[1],
                                     ranks.ctypes.data_as(_capi._ip),
                                     scores.ctypes.data_as(_capi._dp),
                                     n_eff.ctypes.data_as(_capi._ip))
        untouched = (ranks == -77).all() and (scores == -77.0).all() and (n_eff == -77).all()
        return rc, untouched, eng._lib.spfm_last_error(eng._h).decode()

    assert call([0, 1, 1, 1, 1], [5])[:2] == (_capi.SPFM_ERR_INVALID, True)  # no candidates set
    eng.rank_set_candidates(Z, 2, True, False)
    rc, untouched, msg = call([0, 65, 65, 65, 65], np.arange(65))
    assert rc == _capi.SPFM_ERR_UNSUPPORTED and untouched and "SPFM_RANK_MAX_TARGETS = 64" in msg
    bad = [
        ([0, 2, 2, 2, 2], [5, 9], [0, 1, 1, 1, 1], [9]),       # a target that is also excluded
        ([0, 2, 2, 2, 2], [9, 5], None, None),                 # unsorted
        ([0, 2, 2, 2, 2], [5, 5], None, None),                 # duplicate
        ([0, 1, 1, 1, 1], [100], None, None),                  # id out of range
        ([1, 1, 1, 1, 1], [5], None, None),                    # pointers not starting at 0
        ([0, 1, 0, 1, 1], [5], None, None),                    # pointers decreasing
        ([0, 1, 1, 1, 1], [5], [0, 2, 2, 2, 2], [7, 6]),       # unsorted exclusions
    ]
    for tptr, tidx, eptr, eidx in bad:
        assert call(tptr, tidx, eptr, eidx)[:2] == (_capi.SPFM_ERR_INVALID, True), (tptr, tidx)
    # ... and through HipEngine: ValueError / NotImplementedError
    with pytest.raises(NotImplementedError, match="SPFM_RANK_MAX_TARGETS"):
        eng.rank_eval(X, ([0, 65, 65, 65, 65], np.arange(65)))
    with pytest.raises(ValueError, match="excluded"):
        eng.rank_eval(X, ([0, 1, 1, 1, 1], [5]), ([0, 1, 1, 1, 1], [5]))
    with pytest.raises(ValueError, match="ascending"):
        eng.rank_topk(X, 3, exclude=([0, 2, 2, 2, 2], [7, 6]))
    rc, untouched, _ = call([0, 1, 1, 2, 2], [5, 99], [0, 0, 1, 1, 1], [3])
    assert rc == _capi.SPFM_OK and not untouched
    eng.close()


def test_info_and_release():
    from sparsepoly_amd.engine import HipEngine

    est = fm(2, 3, 10)
    X, Z = sides(4, 100, 10)
    eng = HipEngine(0, "f64")
    eng.set_params(est.P_, est.w_, est.lams_)
    eng.rank_set_candidates(Z, 2, True, False)
    before = eng.rank_info()["scratch_kib"]
    lists = ([0, 1, 1, 3, 3], [5, 0, 99]), ([0, 0, 2, 2, 2], [1, 2])
    ranks, scores, n_eff = eng.rank_eval(X, *lists)
    D = eng.rank_scores(X)
    assert (scores == D[[0, 2, 2], [5, 0, 99]]).all() and (n_eff == [100, 98, 100, 100]).all()
    assert ranks[0] == (D[0] > D[0, 5]).sum() + (D[0, :5] == D[0, 5]).sum()
    eng.rank_eval(X, *lists)
    info = eng.rank_info()
    assert info["device_ms"] > 0 and info["scratch_kib"] > before
    # no target at all: nothing runs, n_eff is still answered
    ranks, scores, n_eff = eng.rank_eval(X, ([0, 0, 0, 0, 0], []), ([0, 0, 2, 2, 2], [1, 2]))
    assert ranks.shape == scores.shape == (0,) and (n_eff == [100, 98, 100, 100]).all()
    eng.rank_release()
    assert eng.rank_info()["scratch_kib"] == 0
    with pytest.raises(ValueError, match="rank_set_candidates first"):
        eng.rank_eval(X, ([0, 0, 0, 0, 0], []))
    eng.close()
