"""Negatives of the pairwise fit drawn on the device, host side (no
device): the draw function, the NumPy restatement ``restate_sample``, the argument errors, the
prototypes, and the near-tie cap of every case ``tests/test_hip_pairwise_sample.py`` runs (it
imports its interactions and its helpers from here).  The problem and the cases are those of
``tests/test_pairwise_host.py``."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import ROOT
from test_pairwise_host import CASES, N_CAND, N_CTX, case_id, pair_params, pair_problem

# a chosen negative is compared exactly where the restated best score leads every different
# candidate of its set by this much (1e3 x the margin bar of tests/test_pairwise_host.py) ...
NEAR_TIE = 1e-6
# ... and at most this share of a case's triples may fall below it
NEAR_TIE_SHARE = 0.05
M_VALUES = (3, 8, 33)   # 33: more than one round of L parallel draws at L = 16 and 32
FULL_CTX, FREE_CAND = 5, 13   # context 5 may draw candidate 13 alone


def sample_interactions():
    """(I, E): about 150 positives on the (40, 25) problem and an exclude pattern.  Context 0 (no
    entries) holds exactly one positive; contexts 1 and 2 (70 and 60 entries: the chunked form)
    hold at least two each; context 5 has 24 of its 25 candidates forbidden, most of them through
    ``exclude``; candidate 0 (an empty row) is admissible for most contexts; the number of
    positives is odd, so m is no multiple of the 4 / 8 / 16 groups of a block for n_negatives 1
    and 3."""
    rng = np.random.RandomState(11)
    A = rng.rand(N_CTX, N_CAND) < 0.15
    A[0] = False
    A[0, 7] = True
    for b in (1, 2):
        A[b, [3 * b, 3 * b + 10]] = True
    A[FULL_CTX] = False
    A[FULL_CTX, [2, 20]] = True
    if A.sum() % 2 == 0:
        A[39, 24] = not A[39, 24]
    E = rng.rand(N_CTX, N_CAND) < 0.05
    E[FULL_CTX] = True
    E[FULL_CTX, FREE_CAND] = False
    E[:, 0] = False
    E[FULL_CTX, 0] = True
    return sp.csr_matrix(A.astype(float)), sp.csr_matrix(E.astype(float))


def dense_scores(P, w, lams, X, Z, degree):
    """(B, C) scores s(b, c) in longdouble, by the dense ANOVA evaluation of
    ``restate_margins`` on the summed rows"""
    from sparsepoly_amd.pairwise import _dense_sides, _rows_output

    ld = np.longdouble
    P = np.asarray(P, dtype=ld)
    P = P[None] if P.ndim == 2 else P
    Xd, Zd = _dense_sides(X, Z, ld)
    lin = Zd @ np.asarray(w, dtype=ld)
    return np.stack([_rows_output(P, np.asarray(lams, dtype=ld), Xd[b][None] + Zd, degree)[0] + lin
                     for b in range(X.shape[0])])


def forbidden_dense(I, E):
    F = np.asarray(I.todense()) != 0
    if E is not None:
        F = F | (np.asarray(E.todense()) != 0)
    return F


# ---------------------------------------------------------------- 1. the draw function
def test_draw_u64_is_deterministic_and_keyed_by_all_four_arguments():
    from sparsepoly_amd.pairwise import draw_candidates, draw_u64

    t = np.arange(64, dtype=np.uint64)
    base = draw_u64(5, 2, 9, t)
    assert base.dtype == np.uint64 and base.shape == (64,)
    np.testing.assert_array_equal(base, draw_u64(5, 2, 9, t))
    assert len(np.unique(base)) == 64
    for other in (draw_u64(6, 2, 9, t), draw_u64(5, 3, 9, t), draw_u64(5, 2, 10, t),
                  draw_u64(5, 2, 9, t + np.uint64(64))):
        assert not np.intersect1d(base, other).size
    # scalar and broadcast forms agree
    assert int(draw_u64(5, 2, 9, 3)) == int(base[3])
    r = np.arange(1000, dtype=np.uint64)
    u = draw_u64(123, 0, r[:, None], t[None, :])
    assert u.shape == (1000, 64)
    for C in (1, 2, 25, 20000, 2 ** 31 - 1):
        c = draw_candidates(u, C)
        assert c.min() >= 0 and c.max() < C
    # the restated function, spelled out once more for one value (arithmetic modulo 2**64)
    mask = (1 << 64) - 1

    def mix(z):
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & mask
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    g = 0x9E3779B97F4A7C15
    key = mix(mix((5 << 32) ^ 2) ^ ((9 * g) & mask))
    assert int(base[7]) == mix((key + 8 * g) & mask)


def test_uniform_draws_are_admissible_and_uniform():
    """20 000 draws (n_negatives) of one context with 5 of 25 candidates forbidden, M = 1"""
    from scipy.stats import chi2

    from sparsepoly_amd.pairwise import restate_sample

    X, Z, _ = pair_problem()
    P, w, lams = pair_params(CASES[0])
    I = sp.csr_matrix(([1.0], ([0], [4])), shape=(1, N_CAND))
    E = sp.csr_matrix((np.ones(4), (np.zeros(4, dtype=int), [0, 9, 17, 24])), shape=(1, N_CAND))
    n = 20000
    t, sc, gap = restate_sample(P, w, lams, X[3], Z, I, 2, n, 1, 64, seed=20261020, epoch=0,
                                exclude=E)
    assert t.shape == (n, 3) and (t[:, 0] == 0).all() and (t[:, 1] == 4).all()
    assert not np.isin(t[:, 2], [0, 4, 9, 17, 24]).any()
    assert (sc == 0).all() and np.isinf(gap).all()
    counts = np.bincount(t[:, 2], minlength=N_CAND)
    counts = counts[np.setdiff1d(np.arange(N_CAND), [0, 4, 9, 17, 24])]
    stat = ((counts - n / 20.0) ** 2 / (n / 20.0)).sum()
    print("chi-square over the 20 admissible candidates: %.2f" % stat)
    assert stat < chi2.ppf(1 - 1e-6, 19)


# ---------------------------------------------------------------- 2. restate_sample
def test_restate_sample_properties():
    from sparsepoly_amd.pairwise import restate_sample

    X, Z, _ = pair_problem()
    case = CASES[1]
    P, w, lams = pair_params(case)
    I, E = sample_interactions()
    F = forbidden_dense(I, E)
    assert I.nnz % 2 == 1 and 130 <= I.nnz <= 170
    assert I[0].nnz == 1 and I[1].nnz >= 2 and I[2].nnz >= 2
    assert F[FULL_CTX].sum() == N_CAND - 1 and not F[FULL_CTX, FREE_CAND]
    assert (~F[:, 0]).sum() >= 25
    S = dense_scores(P, w, lams, X, Z, case["degree"])
    rows = np.repeat(np.arange(N_CTX), np.diff(I.indptr))
    for M, max_draws in ((1, 64), (8, 512), (33, 2112), (8, 1), (1, 1)):
        t, sc, gap, det = restate_sample(P, w, lams, X, Z, I, case["degree"], 1, M, max_draws,
                                         seed=77, epoch=3, exclude=E, details=True)
        assert t.dtype == np.int32 and t.shape == (I.nnz, 3)
        np.testing.assert_array_equal(t[:, 0], rows)
        np.testing.assert_array_equal(t[:, 1], I.indices)
        assert not F[t[:, 0], t[:, 2]].any() and (t[:, 1] != t[:, 2]).all()
        # the 24-forbidden context gets its one admissible candidate, by draw or by the walk
        assert (t[rows == FULL_CTX, 2] == FREE_CAND).all()
        for r, (adm, s_adm) in enumerate(det):
            assert 1 <= adm.size <= M and not F[rows[r], adm].any()
            wide = S[rows[r], adm]
            # the chosen score is the maximum over the admitted set (longdouble evaluation)
            assert abs(float(wide.max() - S[rows[r], t[r, 2]])) < 1e-12
            if M > 1:
                assert abs(float(sc[r] - S[rows[r], t[r, 2]])) < 1e-12
            # ties go to the earliest admitted draw
            assert t[r, 2] == adm[np.argmax(s_adm)]
            others = s_adm[adm != t[r, 2]]
            want = np.inf if others.size == 0 else float(s_adm.max() - others.max())
            assert gap[r] == want
        if max_draws == 1:   # at most one admitted draw, else the fallback: one candidate each
            assert all(adm.size == 1 for adm, _ in det) and np.isinf(gap).all()
    # hardest-of-8 does pick something else than the first admitted draw
    t8, _, _, det8 = restate_sample(P, w, lams, X, Z, I, case["degree"], 1, 8, 512, 77, 3,
                                    exclude=E, details=True)
    assert (t8[:, 2] != np.array([adm[0] for adm, _ in det8])).mean() > 0.3
    # exclude matters, seed and epoch matter
    t0 = restate_sample(P, w, lams, X, Z, I, case["degree"], 1, 8, 512, 77, 3)[0]
    assert not np.array_equal(t0, t8)
    for seed, epoch in ((78, 3), (77, 4)):
        assert not np.array_equal(
            t8, restate_sample(P, w, lams, X, Z, I, case["degree"], 1, 8, 512, seed, epoch,
                               exclude=E)[0])


def test_restate_sample_order_permutes_slots_only_and_streams_are_independent():
    from sparsepoly_amd.pairwise import restate_sample

    X, Z, _ = pair_problem()
    case = CASES[4]
    P, w, lams = pair_params(case)
    I, E = sample_interactions()
    m = 3 * I.nnz
    t, sc, gap = restate_sample(P, w, lams, X, Z, I, case["degree"], 3, 8, 512, 1, 0, exclude=E)
    assert t.shape == (m, 3)
    order = np.random.RandomState(0).permutation(m)
    to, sco, gapo = restate_sample(P, w, lams, X, Z, I, case["degree"], 3, 8, 512, 1, 0,
                                   exclude=E, order=order)
    np.testing.assert_array_equal(to[order], t)
    np.testing.assert_array_equal(sco[order], sc)
    np.testing.assert_array_equal(gapo[order], gap)
    # the three negatives of a positive sit side by side and come from streams of their own
    np.testing.assert_array_equal(t[0::3, :2], t[1::3, :2])
    np.testing.assert_array_equal(t[0::3, :2], t[2::3, :2])
    free = np.repeat(N_CAND - forbidden_dense(I, E).sum(axis=1), np.diff(I.indptr))
    wide = free > 12   # (contexts with few admissible candidates repeat themselves)
    assert ((t[0::3, 2] != t[1::3, 2]) | (t[0::3, 2] != t[2::3, 2]))[wide].mean() > 0.5
    tu = restate_sample(P, w, lams, X, Z, I, case["degree"], 3, 1, 64, 1, 0, exclude=E)[0]
    assert (tu[0::3, 2] != tu[1::3, 2])[wide].mean() > 0.8


# ---------------------------------------------------------------- 3. argument errors
def test_sampler_argument_errors_come_before_any_handle(monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker as R
    from sparsepoly_amd import engine, pairwise

    def boom(*a, **k):
        raise AssertionError("a device handle was created")

    monkeypatch.setattr(engine.HipEngine, "__init__", boom)
    monkeypatch.setattr(pairwise._BaseSparseFactorizationMachine, "_new_engine", boom)
    X, Z, t = pair_problem()
    I, E = sample_interactions()
    for sampler in ("uniform", "dynamic"):
        with pytest.raises(ValueError, match="give interactions, not triples"):
            R().fit(X, Z, triples=t, sampler=sampler)
        with pytest.raises(ValueError, match="exactly one"):
            R().fit(X, Z, interactions=I, triples=t, sampler=sampler)
        with pytest.raises(ValueError, match="n_negatives"):
            R().fit(X, Z, interactions=I, sampler=sampler, n_negatives=0)
        with pytest.raises(ValueError, match="row %d stores every candidate" % FULL_CTX):
            full = sp.lil_matrix(E)
            full[FULL_CTX, FREE_CAND] = 1.0
            R().fit(X, Z, interactions=I, sampler=sampler, exclude=sp.csr_matrix(full))
        with pytest.raises(ValueError, match="exclude has shape"):
            R().fit(X, Z, interactions=I, sampler=sampler, exclude=E[:, :5])
    with pytest.raises(ValueError, match="sampler 'nope' is not supported"):
        R().fit(X, Z, interactions=I, sampler="nope")
    with pytest.raises(ValueError, match="sampler 'nope' is not supported"):
        R().fit(X, Z, triples=t, sampler="nope")
    with pytest.raises(ValueError, match="n_candidates"):
        R().fit(X, Z, interactions=I, sampler="dynamic", n_candidates=0)
    est = R()
    with pytest.raises(Exception, match="not fitted"):
        est.sample_negatives(X, Z, I)


# ---------------------------------------------------------------- 4. prototypes
def test_header_capi_and_library_agree_on_the_sampler_symbols():
    import ctypes as C

    from sparsepoly_amd import _capi

    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"spfm_handle": C.c_void_p, "int": C.c_int, "double": C.c_double,
             "int64_t": C.c_int64, "const int32_t*": _capi._ip, "int32_t*": _capi._ip,
             "const int64_t*": _capi._lp, "int64_t*": _capi._lp, "double*": _capi._dp}
    lib = _capi.load()
    for name in ("spfm_psgd_pairs_set_sampler", "spfm_psgd_pairs_sample",
                 "spfm_psgd_pairs_epoch_sampled"):
        m = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        types = [ctype[re.sub(r"\s*\w+$", "", a).replace(" *", "*")] for a in args]
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == types, name


# ---------------------------------------------------------------- 5. the near-tie cap
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_near_ties_of_every_device_case_stay_under_the_cap(case):
    """At the parameters the device cases start from.  Two candidates of one context score within
    1e-6 of each other for context 0 alone (no entries: s(0, c) is a function of the candidate's
    own one or two entries, and the quantised w0 gives two one-entry candidates the same value in
    some cases); every other context keeps its candidates more than 1e-6 apart (the smallest
    distance over the eleven cases, in longdouble: 4.18e-6, k = 30 at degree 4).  Context 0 holds
    one positive, so at most n_negatives triples of a list can sit under the bar."""
    from sparsepoly_amd.pairwise import restate_sample

    X, Z, _ = pair_problem()
    P, w, lams = pair_params(case)
    I, E = sample_interactions()
    S = dense_scores(P, w, lams, X, Z, case["degree"])
    iu = np.triu_indices(N_CAND, 1)
    pair_gap = np.array([np.abs(S[b][:, None] - S[b][None, :])[iu].min() for b in range(N_CTX)])
    print("min candidate gap: context 0 %.3e, the others %.3e"
          % (float(pair_gap[0]), float(pair_gap[1:].min())))
    assert pair_gap[1:].min() > NEAR_TIE
    for M in M_VALUES:
        for n_neg in (1, 3):
            _, _, gap = restate_sample(P, w, lams, X, Z, I, case["degree"], n_neg, M, 64 * M,
                                       seed=4242, epoch=1, exclude=E)
            share = (gap < NEAR_TIE).mean()
            assert share <= n_neg / gap.size <= NEAR_TIE_SHARE, (M, n_neg, share)
