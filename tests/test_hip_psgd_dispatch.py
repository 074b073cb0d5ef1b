"""The lane-width dispatch of the minibatch unit (SPFM_DISPATCH_L: 16 lanes up to k = 16, 32 up to
k = 32, 64 beyond, two component chunks from k = 65) at both sides of each boundary, through
every entry that dispatches on it: the pointwise epoch against the oracle, the pair epoch at one
triple per minibatch against ``restate_pairwise_epoch``, ``psgd_pairs_eval`` against
``restate_margins`` and the dynamic sampler against ``restate_sample``.

12 contexts over 10 candidates, 20 + 20 disjoint columns, 3-6 entries per row, degree 3, one
order, an f64 handle.  The bars are those of tests/test_hip_psgd.py (oracle), tests/test_hip_pairwise.py
(restated epoch, evaluation) and tests/test_hip_pairwise_sample.py (sampler).  The references
are NumPy and C on the host: ``test_references_run_at_every_width`` needs no device."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from test_pairwise_host import MARGIN_ATOL
from test_pairwise_sample_host import NEAR_TIE, NEAR_TIE_SHARE

WIDTHS = (16, 17, 32, 33, 64, 65)
N_CTX, N_CAND, D_SIDE, DEGREE = 12, 10, 20, 3
N_TRIPLES = 40      # one triple per minibatch: one replayed run of 32, then 8 single launches
HYPER = dict(alpha=1e-2, beta=0.5, eta0=0.05, learning_rate="optimal", power_t=0.8)
GAMMA = 0.003
SAMPLE = dict(n_neg=1, M=4, max_draws=64, seed=77, epoch=2)


def _q(v):
    return np.round(v * 64) / 64


@functools.lru_cache(maxsize=None)
def problem():
    rng = np.random.RandomState(3)

    def side(rows, first):
        A = sp.lil_matrix((rows, 2 * D_SIDE))
        for i in range(rows):
            n = rng.randint(3, 7)
            cols = first + rng.choice(D_SIDE, size=n, replace=False)
            A[i, cols] = _q(rng.uniform(0.25, 1.0, size=n)) * np.sign(rng.randn(n))
        return sp.csr_matrix(A)
    X, Z = side(N_CTX, 0), side(N_CAND, D_SIDE)
    t = np.empty((N_TRIPLES, 3), dtype=np.int32)
    t[:, 0] = rng.randint(0, N_CTX, N_TRIPLES)
    t[:, 1] = rng.randint(0, N_CAND, N_TRIPLES)
    t[:, 2] = (t[:, 1] + rng.randint(1, N_CAND, N_TRIPLES)) % N_CAND
    I = sp.csr_matrix(rng.rand(N_CTX, N_CAND) < 0.3, dtype=np.float64)
    I.sort_indices()
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    y = _q(rng.randn(N_CTX + N_CAND))
    order = rng.permutation(N_CTX + N_CAND).astype(np.int32)
    return X, Z, S, y, t, I, order


def params(k):
    rng = np.random.RandomState(100 + k)
    return (_q(0.25 * rng.randn(1, k, 2 * D_SIDE)), _q(0.1 * rng.randn(2 * D_SIDE)),
            np.sign(rng.randn(k)))


@functools.lru_cache(maxsize=None)
def reference(k):
    """what the host says the four entries give at k components (computed once, never changed)"""
    from oracle import oracle as orc
    from sparsepoly_amd.pairwise import (_loss_pos, restate_margins, restate_pairwise_epoch,
                                         restate_sample)

    orc.build()
    orc.lib()
    X, Z, S, y, t, I, order = problem()
    P0, w0, lams = params(k)
    Po, wo = np.ascontiguousarray(P0.swapaxes(1, 2)), w0.copy()
    sl_o, it_o = orc.psgd_epoch(Po, wo, orc.CSR(S), y, lams, DEGREE, HYPER["alpha"], HYPER["beta"],
                                GAMMA, "l1", "squared", order, True, HYPER["eta0"],
                                HYPER["learning_rate"], HYPER["power_t"], 5, 1)
    Pr, wr, slr, itr = restate_pairwise_epoch(P0, w0, lams, X, Z, t, DEGREE, "logistic", "l1",
                                              gamma=GAMMA, batch_size=1, fit_linear=True, it=1,
                                              **HYPER)
    m = restate_margins(P0, w0, lams, X, Z, t, DEGREE)
    ts, sc, gap, det = restate_sample(P0, w0, lams, X, Z, I, DEGREE, SAMPLE["n_neg"], SAMPLE["M"],
                                      SAMPLE["max_draws"], SAMPLE["seed"], SAMPLE["epoch"],
                                      details=True)
    return dict(point=(Po.swapaxes(1, 2).copy(), wo, float(sl_o), it_o),
                pair=(Pr, wr, float(slr), itr),
                margins=m, loss=float(_loss_pos("logistic", m)[0].sum()),
                sample=(ts, sc, gap, det))


def test_references_run_at_every_width():
    """host only: the references exist at all six widths and leave the device comparisons
    meaningful -- every margin clear of zero by 1e3 bars, the near-tie share within its cap"""
    for k in WIDTHS:
        ref = reference(k)
        assert np.isfinite(ref["point"][0]).all() and ref["point"][3] == 1 + 5
        assert np.abs(ref["point"][0] - params(k)[0]).max() > 1e-4
        assert ref["pair"][3] == 1 + N_TRIPLES
        assert np.abs(ref["pair"][0] - params(k)[0]).max() > 1e-4
        assert np.abs(ref["margins"]).min() > 1e3 * MARGIN_ATOL
        ts, sc, gap, det = ref["sample"]
        assert ts.shape == (problem()[5].nnz, 3)
        assert (gap < NEAR_TIE).mean() <= NEAR_TIE_SHARE
        assert sum(int(t[2] != adm[0]) for t, (adm, _) in zip(ts, det)) > 0    # the scores decide


def _engine(k, loss):
    from sparsepoly_amd.engine import HipEngine

    _, _, S, y, _, _, _ = problem()
    P0, w0, lams = params(k)
    eng = HipEngine(0, "f64")
    eng.set_data(S, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", loss, "l1", DEGREE)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("k", WIDTHS)
def test_every_entry_at_the_dispatch_boundaries(k):
    X, Z, S, y, t, I, order = problem()
    ref = reference(k)
    shift = np.array([0, N_CTX, N_CTX], dtype=np.int32)
    ts = (t + shift).astype(np.int32)
    hyper = (DEGREE, HYPER["alpha"], HYPER["beta"], GAMMA, HYPER["eta0"], HYPER["learning_rate"],
             HYPER["power_t"])
    # 1. the pointwise epoch (bars of test_hip_psgd.test_midsize_against_oracle)
    eng = _engine(k, "squared")
    try:
        sl, it = eng.psgd_epoch(*hyper, 5, order, True, 1)
        P, w = eng.get_params()
    finally:
        eng.close()
    Po, wo, sl_o, it_o = ref["point"]
    print("pointwise: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
          % (np.abs(P - Po).max(), np.abs(w - wo).max(), abs(sl - sl_o) / abs(sl_o)))
    assert it == it_o
    np.testing.assert_allclose(sl, sl_o, rtol=1e-11)
    np.testing.assert_allclose(P, Po, rtol=0, atol=1e-10)
    np.testing.assert_allclose(w, wo, rtol=0, atol=1e-10)
    eng = _engine(k, "logistic")
    try:
        # 2. evaluation at the initial parameters (bars of test_pairs_eval_reads_and_changes_nothing)
        sl, n_ord = eng.psgd_pairs_eval(DEGREE, True, ts)
        print("eval: rel dloss = %.3e" % (abs(sl - ref["loss"]) / abs(ref["loss"])))
        np.testing.assert_allclose(sl, ref["loss"], rtol=1e-10)
        assert n_ord == int((ref["margins"] > 0).sum())
        # 3. the sampler, hardest of 4 (the rule of test_hip_pairwise_sample.check_dynamic)
        eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I)
        m, td, scd = eng.psgd_pairs_sample(DEGREE, SAMPLE["n_neg"], SAMPLE["M"],
                                           SAMPLE["max_draws"], SAMPLE["seed"], SAMPLE["epoch"])
        tr, _, gap, det = ref["sample"]
        got = td - shift
        assert m == I.nnz
        np.testing.assert_array_equal(got[:, :2], tr[:, :2])
        clear = gap >= NEAR_TIE
        worst = 0.0
        for r, (adm, s_adm) in enumerate(det):
            c = got[r, 2]
            assert c in adm, (r, c, adm)
            s_c = s_adm[list(adm).index(c)]
            assert s_c >= s_adm.max() - NEAR_TIE
            worst = max(worst, abs(float(scd[r] - s_c)))
        print("sample: m = %d, near-tie share %.4f, max |score - restated| = %.3e"
              % (m, 1.0 - clear.mean(), worst))
        np.testing.assert_array_equal(got[clear, 2], tr[clear, 2])
        assert worst <= MARGIN_ATOL
        assert 1.0 - clear.mean() <= NEAR_TIE_SHARE
        # 4. the pair epoch, one triple per minibatch (bars of
        #    test_hip_pairwise.test_one_and_two_epochs_against_the_restatement)
        sl, it = eng.psgd_pairs_epoch(*hyper, 1, ts, True, 1)
        P, w = eng.get_params()
    finally:
        eng.close()
    Pr, wr, slr, itr = ref["pair"]
    print("pair epoch: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
          % (np.abs(P - Pr).max(), np.abs(w - wr).max(), abs(sl - slr) / abs(slr)))
    assert it == itr
    np.testing.assert_allclose(sl, slr, rtol=1e-10)
    np.testing.assert_allclose(P, Pr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(w, wr, rtol=0, atol=1e-9)
