"""Weighted triples, proposal draws and the WARP sampler on the device
against the NumPy restatements.  Needs a real MI355X: ``pytest -m gpu``.  The problem and the
cases come from ``tests/test_pairwise_host.py``, the interactions from
``tests/test_pairwise_sample_host.py``, the parameters and margins of the WARP cases from
``tests/test_pairwise_warp_host.py`` (which asserts their coverage and near-tie cap on the host).

The draws are integer arithmetic and are compared exactly.  WARP's negative and trial count are
compared exactly wherever every tried candidate's restated score keeps ``NEAR_TIE`` = 1e-6 from
the threshold (and, without a violator, the best score leads by as much); elsewhere the device may
differ within that distance.  The epochs are held to the project's psgd bars."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from test_hip_pairwise_sample import (E2E_EPOCHS, E2E_KW, P_ATOL, SHIFT, SL_RTOL, _engine, _hyper,
                                      planted_problem)
from test_pairwise_host import (CASES, GAMMA, HYPER, MARGIN_ATOL, N_CAND, N_CTX, _case, case_id,
                                pair_params, pair_problem)
from test_pairwise_sample_host import (FREE_CAND, FULL_CTX, M_VALUES, NEAR_TIE, NEAR_TIE_SHARE,
                                       forbidden_dense, sample_interactions)
from test_pairwise_warp_host import (WARP_EPOCH, WARP_SEED, _draw_params, spread_margin,
                                     triple_weights, warp_params)

pytestmark = pytest.mark.gpu


def _weights(m):
    return np.resize(triple_weights(), m)


def _table(zeros=(1, 4, 9, 16)):
    """(candidate weights, cum): count ** 0.75-like weights with some candidates at 0"""
    from sparsepoly_amd.pairwise import proposal_cum, quantise_proposal

    w = (np.arange(N_CAND) % 7 + 1.0) ** 0.75
    w[list(zeros)] = 0.0
    return w, proposal_cum(quantise_proposal(w, N_CAND))


def _epoch_w(eng, case, ts, wt, it):
    return eng.psgd_pairs_epoch_weighted(*_hyper(case), ts, wt, case["fit_linear"], it)


@functools.lru_cache(maxsize=None)
def _weighted_ref(ci, n_epochs, batch=None, reg=None):
    """[(P, w, sum_loss, it) after each epoch] of a case under the test weights; computed once
    per process and shared -- treat every array as read-only"""
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    case = dict(CASES[ci])
    if batch:
        case["batch"] = batch
    if reg:
        case["reg"] = reg
    X, Z, t = pair_problem()
    t = t[:case["n_triples"]]
    P, w, lams = pair_params(case)
    it, out = 1, []
    for _ in range(n_epochs):
        P, w, sl, it = restate_pairwise_epoch(
            P, w, lams, X, Z, t, case["degree"], case["loss"], case["reg"],
            gamma=GAMMA[case["reg"]], batch_size=case["batch"], fit_linear=case["fit_linear"],
            it=it, weights=_weights(len(t)), **HYPER)
        out.append((P, w, float(sl), it))
    return case, (X, Z, t, lams), out


# ------------------------------------------------------------------ 1. the weighted epoch
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_weighted_epochs_against_the_restatement(ci):
    case, (X, Z, t, lams), ref = _weighted_ref(ci, 2)
    ts = (t + SHIFT).astype(np.int32)
    wt = _weights(len(t))
    assert (wt == 0).any() and (wt == 1).any() and (wt != np.floor(wt)).any()
    prec = case["precision"]
    eng = _engine(case, X, Z, sampler=False)
    it = 1
    try:
        for ep in range(2):
            sl, it = _epoch_w(eng, case, ts, wt, it)
            P, w = eng.get_params()
            Pr, wr, slr, itr = ref[ep]
            print("epoch %d: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
                  % (ep + 1, np.abs(P - Pr).max(), np.abs(w - wr).max(), abs(sl - slr) / abs(slr)))
            assert it == itr
            np.testing.assert_allclose(sl, slr, rtol=SL_RTOL[prec])
            np.testing.assert_allclose(P, Pr, rtol=0, atol=P_ATOL[prec])
            np.testing.assert_allclose(w, wr, rtol=0, atol=P_ATOL[prec])
        assert np.abs(P - pair_params(case)[0]).max() > 1e-4     # it did train
    finally:
        eng.close()


@pytest.mark.parametrize("ci", [0, 1, 2, 3, 4, 7],
                         ids=[case_id(CASES[c]) for c in (0, 1, 2, 3, 4, 7)])
def test_all_ones_weights_keep_the_bits_of_the_plain_epoch(ci):
    """One triple per minibatch: at most two atomics of a launch meet at an address (a column
    c+ and c- share) and a sum of two terms from zero does not depend on their order, so both
    routes are functions of their inputs and are compared bit for bit; the cases' own batch size
    at the psgd bar."""
    X, Z, t = pair_problem()
    ts = (t + SHIFT).astype(np.int32)
    for batch in (1, CASES[ci]["batch"]):
        case = dict(CASES[ci], batch=batch)
        res = []
        for weighted in (False, True):
            eng = _engine(case, X, Z, sampler=False)
            try:
                it, sls = 1, []
                for _ in range(2):
                    if weighted:
                        sl, it = _epoch_w(eng, case, ts, np.ones(len(ts)), it)
                    else:
                        sl, it = eng.psgd_pairs_epoch(*_hyper(case), ts, case["fit_linear"], it)
                    sls.append(sl)
                res.append((eng.get_params(), sls, it))
            finally:
                eng.close()
        (Pa, wa), sla, ita = res[0]
        (Pb, wb), slb, itb = res[1]
        assert ita == itb and np.isfinite(Pa).all() and np.isfinite(Pb).all()
        print("batch %d: max|dP| = %.3e" % (batch, np.abs(Pa - Pb).max()))
        if batch == 1:
            assert np.array_equal(Pa, Pb) and np.array_equal(wa, wb)
            np.testing.assert_allclose(sla, slb, rtol=1e-14)   # (the loss sum is a tree of its own)
        else:
            prec = case["precision"]
            np.testing.assert_allclose(Pa, Pb, rtol=0, atol=P_ATOL[prec])
            np.testing.assert_allclose(wa, wb, rtol=0, atol=P_ATOL[prec])
            np.testing.assert_allclose(sla, slb, rtol=SL_RTOL[prec])


@pytest.mark.parametrize("reg", ["l1", "squaredl12"])
def test_weighted_graph_replay_agrees_with_eager_launches(reg):
    """38 minibatches per epoch: one replayed run of 32 and 6 single launches (the table route
    offsets the weights by the batch position like the triples and the losses)"""
    case, (X, Z, t, lams), ref = _weighted_ref(1, 3, batch=4, reg=reg)
    ts = (t + SHIFT).astype(np.int32)
    wt = _weights(len(t))
    res = {}
    for mode, opts in (("graph", ()), ("eager", (("psgd_eager", 1),))):
        eng = _engine(case, X, Z, sampler=False)
        for key, val in opts:
            eng.set_option(key, val)
        it, sls = 1, []
        for _ in range(3):
            sl, it = _epoch_w(eng, case, ts, wt, it)
            sls.append(sl)
        res[mode] = (eng.get_params(), np.array(sls), it, eng.get_option("psgd_redone"))
        eng.close()
    assert res["eager"][3] == 0
    for mode in res:
        (P, w), sls, it, _ = res[mode]
        assert it == ref[2][3] == 1 + 3 * 38
        np.testing.assert_allclose(sls, [r[2] for r in ref], rtol=1e-10, err_msg=mode)
        np.testing.assert_allclose(P, ref[2][0], rtol=0, atol=1e-9, err_msg=mode)
        np.testing.assert_allclose(w, ref[2][1], rtol=0, atol=1e-9, err_msg=mode)
    np.testing.assert_allclose(res["graph"][0][0], res["eager"][0][0], rtol=0, atol=1e-9)


# ------------------------------------------------------------------ 2. the proposal table
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("k_case", [0, 1, 2, 3], ids=["k5", "k30", "k40", "k70"])
def test_uniform_sampler_with_a_table_is_exact(k_case, precision):
    from sparsepoly_amd.pairwise import restate_sample

    case = dict(CASES[k_case], precision=precision)
    X, Z, _ = pair_problem()
    P, w, lams = pair_params(case)
    I, E = sample_interactions()
    F = forbidden_dense(I, E)
    zeros = (1, 4, 9, 16)
    _, cum = _table(zeros)
    eng = _engine(case, X, Z)
    try:
        plain = eng.psgd_pairs_sample(case["degree"], 3, 1, 64, 99, 4)[1]
        eng.psgd_pairs_set_proposal(cum)
        for n_neg, max_draws, shuffled in ((1, 64, False), (3, 64, True), (3, 1, False),
                                           (1, 1, True)):
            m = I.nnz * n_neg
            order = np.random.RandomState(m).permutation(m) if shuffled else None
            got_m, t, sc = eng.psgd_pairs_sample(case["degree"], n_neg, 1, max_draws, 99, 4, order)
            want, _, _ = restate_sample(P, w, lams, X, Z, I, case["degree"], n_neg, 1, max_draws,
                                        99, 4, exclude=E, order=order, cum=cum)
            assert got_m == m
            np.testing.assert_array_equal(t - SHIFT, want)
            assert (sc == 0).all()
            assert not F[t[:, 0], t[:, 2] - N_CTX].any()
            assert (t[t[:, 0] == FULL_CTX, 2] == N_CTX + FREE_CAND).all()
            if max_draws == 64:    # (FREE_CAND apart, which the walk reaches) weight 0: never drawn
                free = t[:, 0] != FULL_CTX
                assert not np.isin(t[free, 2] - N_CTX, zeros).any()
        assert not np.array_equal(eng.psgd_pairs_sample(case["degree"], 3, 1, 64, 99, 4)[1], plain)
        eng.psgd_pairs_set_proposal(None)      # NULL: today's draws again, exactly
        np.testing.assert_array_equal(eng.psgd_pairs_sample(case["degree"], 3, 1, 64, 99, 4)[1],
                                      plain)
        after = eng.get_params()
        assert np.array_equal(after[0], P) and np.array_equal(after[1], w)
    finally:
        eng.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[6], CASES[8]], ids=case_id)
def test_dynamic_sampler_with_a_table_against_the_restatement(case):
    """the near-tie rule of tests/test_hip_pairwise_sample.py"""
    from sparsepoly_amd.pairwise import restate_sample

    X, Z, _ = pair_problem()
    P, w, lams = pair_params(case)
    I, E = sample_interactions()
    _, cum = _table()
    eng = _engine(case, X, Z)
    try:
        eng.psgd_pairs_set_proposal(cum)
        _, t_dev, sc_dev = eng.psgd_pairs_sample(case["degree"], 1, 8, 512, 4242, 1)
    finally:
        eng.close()
    t, sc, gap, det = restate_sample(P, w, lams, X, Z, I, case["degree"], 1, 8, 512, 4242, 1,
                                     exclude=E, details=True, cum=cum)
    got = t_dev - SHIFT
    np.testing.assert_array_equal(got[:, :2], t[:, :2])
    clear = gap >= NEAR_TIE
    worst = 0.0
    for r, (adm, s_adm) in enumerate(det):
        c = got[r, 2]
        assert c in adm, (r, c, adm)
        s_c = s_adm[list(adm).index(c)]
        assert s_c >= s_adm.max() - NEAR_TIE
        worst = max(worst, abs(float(sc_dev[r] - s_c)))
    print("near-tie share %.4f, max |score - restated| = %.3e" % (1 - clear.mean(), worst))
    np.testing.assert_array_equal(got[clear, 2], t[clear, 2])
    assert worst <= MARGIN_ATOL and 1 - clear.mean() <= NEAR_TIE_SHARE


# ------------------------------------------------------------------ 3. WARP
def check_warp(dev, P, w, lams, X, Z, degree, n_neg, M, max_draws, margin, seed, epoch,
               order=None, cum=None, posw=None):
    """the rule of the WARP comparison; returns the restated (triples, weights, trials) by slot
    and the share of triples that are not compared exactly"""
    from sparsepoly_amd.pairwise import restate_warp

    t_dev, sc_dev, wt_dev, tr_dev = dev
    I, E = sample_interactions()
    t, sc, wt, tr, near, det = restate_warp(P, w, lams, X, Z, I, degree, n_neg, M, max_draws,
                                            margin, seed, epoch, exclude=E, order=order, cum=cum,
                                            positive_weights=posw, details=True)
    m = t.shape[0]
    slots = np.arange(m) if order is None else np.asarray(order)
    got = t_dev - SHIFT
    np.testing.assert_array_equal(got[:, :2], t[:, :2])
    clear = near >= NEAR_TIE
    for r, (adm, s_adm, thr) in enumerate(det):
        s = slots[r]
        if tr[s] == 0 and adm.size:     # no violator: the best of those tried must lead as well
            others = s_adm[adm != t[s, 2]]
            if others.size and float(s_adm.max() - others.max()) < NEAR_TIE:
                clear[s] = False
        if not clear[s] and adm.size:   # within the distance: any candidate the rule allows
            assert got[s, 2] in adm
    np.testing.assert_array_equal(got[clear, 2], t[clear, 2])
    np.testing.assert_array_equal(tr_dev[clear], tr[clear])
    np.testing.assert_allclose(wt_dev[clear], wt[clear], rtol=1e-12, atol=0)
    worst = np.abs(sc_dev[clear] - sc[clear].astype(np.double)).max()
    share = 1.0 - clear.mean()
    print("M = %d, margin %.4f: trials 0 / 1 / 2-4 / >4 / >16 = %d / %d / %d / %d / %d, "
          "unclear share %.4f, max |score - restated| = %.3e"
          % (M, margin, (tr == 0).sum(), (tr == 1).sum(), ((tr > 1) & (tr <= 4)).sum(),
             (tr > 4).sum(), (tr > 16).sum(), share, worst))
    assert worst <= MARGIN_ATOL
    assert (wt_dev[tr_dev == 0] == 0).all() and (wt_dev >= 0).all()
    return (t, wt, tr), share


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_warp_sampler_against_the_restatement(case):
    """both margins and n_candidates = 3 / 8 / 33; positive weights at 8 (the product), an
    `order` at 33"""
    X, Z, _ = pair_problem()
    P, w, lams, spread = warp_params(case)
    I, _ = sample_interactions()
    posw = 0.25 + np.arange(I.nnz) % 5
    eng = _engine(case, X, Z, params=(P, w, lams))
    seen = np.zeros(5, dtype=bool)
    try:
        for margin in (0.0, spread):
            for M in M_VALUES:
                n_neg = 3 if M == 3 else 1
                m = I.nnz * n_neg
                order = np.random.RandomState(M).permutation(m) if M == 33 else None
                eng.psgd_pairs_set_positive_weights(posw if M == 8 else None)
                got_m, *dev = eng.psgd_pairs_sample_warp(case["degree"], n_neg, M, 64 * M, margin,
                                                         WARP_SEED, WARP_EPOCH, order)
                assert got_m == m
                (_, _, tr), share = check_warp(dev, P, w, lams, X, Z, case["degree"], n_neg, M,
                                               64 * M, margin, WARP_SEED, WARP_EPOCH, order,
                                               posw=posw if M == 8 else None)
                assert share <= NEAR_TIE_SHARE
                seen |= [(tr == 0).any(), (tr == 1).any(), ((tr > 1) & (tr <= 4)).any(),
                         (tr > 4).any(), (tr > 16).any()]
        assert seen.all()       # (asserted on the host already: the comparison saw every class)
        after = eng.get_params()
        assert np.array_equal(after[0], P) and np.array_equal(after[1], w)
    finally:
        eng.close()


CHUNKED = _case(70, 3, "explicit", True, "l1", "logistic", 47)


def test_warp_sampler_in_the_chunked_form_with_a_table():
    """k = 70 (two component chunks at L = 64), two orders, and the positives of contexts 1 and 2
    (70 and 60 entries: more than one chunk of 64); a proposal table and max_draws = 1 (the
    fallback) on top"""
    X, Z, _ = pair_problem()
    P, w, lams = _draw_params(CHUNKED, 5)
    margin = spread_margin(P, w, lams, X, Z, 3)
    I, _ = sample_interactions()
    assert I[1].nnz >= 2 and X[1].nnz > 64
    _, cum = _table()
    eng = _engine(CHUNKED, X, Z, params=(P, w, lams))
    try:
        for M, max_draws, table in ((8, 512, None), (33, 2112, cum), (1, 1, cum), (3, 3, None)):
            eng.psgd_pairs_set_proposal(table)
            _, *dev = eng.psgd_pairs_sample_warp(3, 1, M, max_draws, margin, 9, 2)
            _, share = check_warp(dev, P, w, lams, X, Z, 3, 1, M, max_draws, margin, 9, 2,
                                  cum=table)
            assert share <= NEAR_TIE_SHARE
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. sampled == uploaded
@pytest.mark.parametrize("case", [dict(CASES[1], batch=4), CASES[7]], ids=case_id)
def test_warp_sampled_epoch_equals_weighted_uploaded_epoch(case):
    """three epochs, each from the parameters downloaded at its start; batch = 4: 38 minibatches
    per epoch, one replayed run of 32 among them.  The third epoch samples plainly with positive
    weights: the weights left on the device are the positives' own."""
    X, Z, _ = pair_problem()
    P0, w0, lams, spread = warp_params(CASES[1] if case["k"] == 30 and case["batch"] == 4
                                       else case)
    prec = case["precision"]
    I, _ = sample_interactions()
    posw = 0.25 + np.arange(I.nnz) % 5
    a = _engine(case, X, Z, params=(P0, w0, lams))
    try:
        a.psgd_pairs_set_positive_weights(posw)
        it = 1
        for ep in range(3):
            P, w = a.get_params()
            order = np.random.RandomState(ep).permutation(I.nnz)
            if ep < 2:
                m, t, _, wt, tr = a.psgd_pairs_sample_warp(case["degree"], 1, 8, 512, spread, 7,
                                                           ep, order)
                assert (wt == 0).any() and (wt > 0).any() and (tr[wt > 0] > 0).all()
            else:
                m, t, _ = a.psgd_pairs_sample(case["degree"], 1, 8, 512, 7, ep, order)
                wt = np.empty(m)
                wt[order] = posw
            sl_a, it_a = a.psgd_pairs_epoch_sampled(*_hyper(case), case["fit_linear"], it)
            b = _engine(case, X, Z, params=(P, w, lams), sampler=False)
            try:
                sl_b, it_b = _epoch_w(b, case, t, wt, it)
                Pb, wb = b.get_params()
            finally:
                b.close()
            Pa, wa = a.get_params()
            print("epoch %d: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
                  % (ep + 1, np.abs(Pa - Pb).max(), np.abs(wa - wb).max(),
                     abs(sl_a - sl_b) / abs(sl_b)))
            assert it_a == it_b == it + -(-m // case["batch"])
            np.testing.assert_allclose(sl_a, sl_b, rtol=SL_RTOL[prec])
            np.testing.assert_allclose(Pa, Pb, rtol=0, atol=P_ATOL[prec])
            np.testing.assert_allclose(wa, wb, rtol=0, atol=P_ATOL[prec])
            assert np.abs(Pa - P).max() > 1e-6     # it did train
            it = it_a
    finally:
        a.close()


# ------------------------------------------------------------------ 5. error codes
def test_error_codes_behind_the_c_abi():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    INV, OK = _capi.SPFM_ERR_INVALID, _capi.SPFM_OK
    case = CASES[0]
    X, Z, tr = pair_problem()
    I, E = sample_interactions()
    ts = (tr + SHIFT).astype(np.int32)
    _, cum = _table()
    eng = _engine(case, X, Z, sampler=False)
    lib, h = eng._lib, eng._h
    up = C.POINTER(C.c_uint32)

    def epoch_w(weights, triples=ts, handle=None, batch=8):
        wt = np.ascontiguousarray(weights, dtype=np.float64)
        itc, sl = C.c_int64(1), C.c_double()
        return lib.spfm_psgd_pairs_epoch_weighted(
            handle or h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, batch,
            triples.ctypes.data_as(_capi._ip), wt.ctypes.data_as(_capi._dp), triples.shape[0], 1,
            C.byref(itc), C.byref(sl))

    def set_proposal(c, n=None, handle=None):
        c = np.ascontiguousarray(c, dtype=np.uint32)
        return lib.spfm_psgd_pairs_set_proposal(handle or h, c.ctypes.data_as(up),
                                                c.size if n is None else n)

    def set_posw(v, n=None, handle=None):
        v = np.ascontiguousarray(v, dtype=np.float64)
        return lib.spfm_psgd_pairs_set_positive_weights(handle or h, v.ctypes.data_as(_capi._dp),
                                                        v.size if n is None else n)

    def warp(M=4, max_draws=64, margin=0.0, degree=2, n_neg=1, handle=None):
        return lib.spfm_psgd_pairs_sample_warp(handle or h, degree, n_neg, M, max_draws, margin, 1,
                                               0, None, None, None, None, None)

    def lists_sampled():
        itc, sl = C.c_int64(1), C.c_double()
        return lib.spfm_psgd_lists_epoch_sampled(h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, 8, 1, 0,
                                                 None, 1, C.byref(itc), C.byref(sl))

    before = eng.get_params()
    ones = np.ones(len(ts))
    # bad weights, and what the plain epoch rejects
    for bad in (-1.0, np.nan, np.inf):
        wt = ones.copy()
        wt[17] = bad
        assert epoch_w(wt) == INV
    worse = ts.copy()
    worse[3, 2] = worse[3, 1]
    assert epoch_w(ones, worse) == INV
    assert epoch_w(ones, batch=0) == INV
    # the set calls without a sampler
    assert set_proposal(cum) == INV and set_posw(np.ones(I.nnz)) == INV
    assert lib.spfm_psgd_pairs_set_proposal(h, None, 0) == INV
    assert warp() == INV
    eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I, I + E)
    # bad cum, wrong lengths, bad positive weights
    assert set_proposal(cum[:-1]) == INV
    down = cum.copy()
    down[5] = down[4] - 1
    assert set_proposal(down) == INV
    assert set_proposal(np.zeros(N_CAND)) == INV
    assert set_posw(np.ones(I.nnz - 1)) == INV
    for bad in (-0.5, np.nan, np.inf):
        v = np.ones(I.nnz)
        v[3] = bad
        assert set_posw(v) == INV
    assert set_proposal(cum) == OK and lib.spfm_psgd_pairs_set_proposal(h, None, 0) == OK
    # the WARP call's own arguments, and those of the plain sample call
    assert warp(M=0) == INV
    assert warp(M=65, max_draws=64) == INV
    assert warp(margin=np.inf) == INV and warp(margin=np.nan) == INV
    assert warp(degree=3) == INV and warp(n_neg=0) == INV and warp(max_draws=0) == INV
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # the lists epoch after a weighted sample; after a plain one it runs
    assert warp() == OK
    assert lists_sampled() == INV
    with pytest.raises(ValueError, match="wrote weights"):
        eng.psgd_lists_epoch_sampled(2, 0.01, 0.5, 0.003, 0.05, "optimal", 0.8, 8, 1, "softmax",
                                     True, 1)
    assert set_posw(np.ones(I.nnz)) == OK
    eng.psgd_pairs_sample(2, 1, 4, 64, 1, 0, want_triples=False, want_scores=False)
    assert lists_sampled() == INV
    after = eng.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert lib.spfm_psgd_pairs_set_positive_weights(h, None, 0) == OK
    eng.psgd_pairs_sample(2, 1, 4, 64, 1, 0, want_triples=False, want_scores=False)
    assert lists_sampled() == OK
    # a new sampler drops the table and the weights: the draws are the plain ones again
    plain = eng.psgd_pairs_sample(2, 1, 1, 64, 1, 0)[1]
    assert set_proposal(cum) == OK
    assert not np.array_equal(eng.psgd_pairs_sample(2, 1, 1, 64, 1, 0)[1], plain)
    eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I, I + E)
    np.testing.assert_array_equal(eng.psgd_pairs_sample(2, 1, 1, 64, 1, 0)[1], plain)
    eng.close()


def test_a_handle_with_a_communicator_is_unsupported():
    """a 1-rank communicator makes the handle a distributed one: the weighted epoch and the WARP
    sample call answer SPFM_ERR_UNSUPPORTED before anything else and leave the parameters as they
    were"""
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    UNS = _capi.SPFM_ERR_UNSUPPORTED
    case = CASES[0]
    X, Z, tr = pair_problem()
    I, E = sample_interactions()
    ts = (tr + SHIFT).astype(np.int32)
    ones = np.ones(len(ts))
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    P0, w0, lams = pair_params(case)
    eng = HipEngine(0, "f64")
    try:
        eng.comm_init(HipEngine.comm_unique_id(), 1, 0)
        eng.set_data(S, np.zeros(S.shape[0]))
        eng.set_params(P0.copy(), w0.copy(), lams)
        eng.configure("psgd", case["loss"], case["reg"], case["degree"])
        eng.psgd_pairs_set_sampler(N_CTX, N_CAND, I, I + E)
        itc, sl = C.c_int64(1), C.c_double()
        assert eng._lib.spfm_psgd_pairs_epoch_weighted(
            eng._h, 2, 0.01, 0.5, 0.003, 0.05, 1, 0.8, 8, ts.ctypes.data_as(_capi._ip),
            ones.ctypes.data_as(_capi._dp), ts.shape[0], 1, C.byref(itc), C.byref(sl)) == UNS
        assert eng._lib.spfm_psgd_pairs_sample_warp(
            eng._h, 2, 1, 4, 64, 0.0, 1, 0, None, None, None, None, None) == UNS
        after = eng.get_params()
        assert np.array_equal(P0, after[0]) and np.array_equal(w0, after[1])
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. the estimator
WARM_KW = dict(E2E_KW, eta0=0.05, learning_rate="optimal", power_t=0.8, alpha=1e-2, beta=0.5,
               gamma=0.003, warm_start=True)


def _warm(est, d, seed=5):
    """parameters of the size the device cases use (at the 0.01-scale initialisation and margin
    1 every first trial violates, which would test nothing)"""
    rng = np.random.RandomState(seed)
    est.P_ = 0.25 * rng.randn(1, 6, d)     # (not quantised: the f64 handle keeps them, and
    est.w_ = 0.1 * rng.randn(d)            # quantised products tie exactly at margin 0)
    est.lams_ = np.ones(6)
    return est.P_.copy(), est.w_.copy()


def _fit_and_starts(fit_kw, X, Z):
    from sparsepoly_amd import SparseFactorizationMachineRanker

    seen = []
    est = SparseFactorizationMachineRanker(
        callback=lambda e: seen.append((e.P_.copy(), e.w_.copy())), n_calls=1, **WARM_KW)
    P0, w0 = _warm(est, X.shape[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit(X, Z, **fit_kw)
    assert len(seen) == E2E_EPOCHS
    return est, seen, [(P0, w0)] + seen[:-1]


def _restated_epoch(P, w, X, Z, t, it, weights):
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    return restate_pairwise_epoch(P, w, np.ones(6), X, Z, t, 2, "logistic", "l1", 1e-2, 0.5, 0.003,
                                  0.05, "optimal", 0.8, 64, True, it, weights=weights)


def test_ranker_fit_with_the_warp_sampler():
    """the fit against the loop rebuilt from restate_warp + restate_pairwise_epoch under the same
    random_state, every epoch from the parameters a callback read off the device"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd.pairwise import restate_warp

    X, Z, train, held = planted_problem()
    vals = sp.csr_matrix(train, copy=True)
    vals.sort_indices()
    vals.data = 0.5 + np.arange(vals.nnz) % 4          # the interactions' own values
    est, seen, starts = _fit_and_starts(
        dict(interactions=vals, n_negatives=2, resample=True, sampler="warp", n_candidates=4,
             margin=0.0, exclude=held, sample_weight="data"), X, Z)
    rng = check_random_state(WARM_KW["random_state"])
    seed = rng.randint(0, 2 ** 31 - 1)     # warm start: no parameter is drawn before it
    m = train.nnz * 2
    it = 1
    n_zero = 0
    for ep, (P, w) in enumerate(starts):
        order = rng.permutation(m)
        t, _, wt, tr, near, det = restate_warp(P, w, np.ones(6), X, Z, train, 2, 2, 4, 256, 0.0,
                                               seed, ep, exclude=held, order=order,
                                               positive_weights=vals.data, details=True)
        # the epoch can only be compared if the device drew the restated list: its scores meet
        # MARGIN_ATOL, so thresholds (and best scores) that lead by twice that fix the choices
        assert near.min() > 2 * MARGIN_ATOL, near.min()
        for r, (adm, s_adm, thr) in enumerate(det):
            if tr[order[r]] == 0 and adm.size > 1:
                top = np.sort(s_adm[np.unique(adm, return_index=True)[1]])
                assert top.size < 2 or top[-1] - top[-2] > 2 * MARGIN_ATOL
        n_zero += int((tr == 0).sum())
        Pr, wr, _, it = _restated_epoch(P, w, X, Z, t, it, wt)
        np.testing.assert_allclose(seen[ep][0], Pr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(seen[ep][1], wr, rtol=0, atol=1e-9)
    assert 0 < n_zero < 3 * m       # some triples found no violator, most did
    assert est.it_ == it == 1 + E2E_EPOCHS * 25


def test_ranker_fit_with_popularity_proposal_and_data_weights():
    """proposal='popularity' with the uniform sampler and sample_weight='data' on the device
    route; sample_weight on the host route and with explicit triples"""
    from sklearn.utils import check_random_state

    from sparsepoly_amd.pairwise import (epoch_triples, popularity_weights, proposal_cum,
                                         quantise_proposal, restate_sample)

    X, Z, train, held = planted_problem()
    vals = sp.csr_matrix(train, copy=True)
    vals.sort_indices()
    vals.data = 0.5 + np.arange(vals.nnz) % 4
    m = train.nnz * 2
    # device route
    est, seen, starts = _fit_and_starts(
        dict(interactions=vals, n_negatives=2, sampler="uniform", exclude=held,
             proposal="popularity", proposal_power=0.5, sample_weight="data"), X, Z)
    pop = (np.bincount(train.indices, minlength=train.shape[1]) + 1.0) ** 0.5
    np.testing.assert_array_equal(popularity_weights(train, 0.5), pop)
    cum = proposal_cum(quantise_proposal(pop))
    rng = check_random_state(WARM_KW["random_state"])
    seed = rng.randint(0, 2 ** 31 - 1)
    it = 1
    for ep, (P, w) in enumerate(starts):
        order = rng.permutation(m)
        t, _, _ = restate_sample(P, w, np.ones(6), X, Z, train, 2, 2, 1, 64, seed, ep,
                                 exclude=held, order=order, cum=cum)
        wt = np.empty(m)
        wt[order] = np.repeat(vals.data, 2)
        Pr, wr, _, it = _restated_epoch(P, w, X, Z, t, it, wt)
        np.testing.assert_allclose(seen[ep][0], Pr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(seen[ep][1], wr, rtol=0, atol=1e-9)
    assert est.it_ == it
    # host route
    est, seen, starts = _fit_and_starts(
        dict(interactions=vals, n_negatives=2, exclude=held, sample_weight="data"), X, Z)
    lists = epoch_triples(check_random_state(WARM_KW["random_state"]), E2E_EPOCHS, train, None, 2,
                          True, True, held, weights=vals.data)
    it = 1
    for ep, ((P, w), (t, wt)) in enumerate(zip(starts, lists)):
        Pr, wr, _, it = _restated_epoch(P, w, X, Z, t, it, wt)
        np.testing.assert_allclose(seen[ep][0], Pr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(seen[ep][1], wr, rtol=0, atol=1e-9)
    # explicit triples
    t0, wt0 = next(epoch_triples(check_random_state(1), 1, train, None, 2, True, False, held,
                                 weights=vals.data))
    est, seen, starts = _fit_and_starts(dict(triples=t0, sample_weight=wt0), X, Z)
    perm_rng = check_random_state(WARM_KW["random_state"])
    it = 1
    for ep, (P, w) in enumerate(starts):
        perm = perm_rng.permutation(m)
        Pr, wr, _, it = _restated_epoch(P, w, X, Z, t0[perm], it, wt0[perm])
        np.testing.assert_allclose(seen[ep][0], Pr, rtol=0, atol=1e-9)
        np.testing.assert_allclose(seen[ep][1], wr, rtol=0, atol=1e-9)
    # the weights matter
    plain = _fit_and_starts(dict(triples=t0), X, Z)[0]
    assert np.abs(plain.P_ - est.P_).max() > 1e-6


def test_default_keywords_keep_the_bits_and_the_errors_are_raised():
    """one triple per minibatch (see test_host_sampler_keeps_its_bits_and_honours_exclude of
    tests/test_hip_pairwise_sample.py): a fit with every new keyword at its default against a
    fit without them, bit for bit, on the host and the dynamic route"""
    from sparsepoly_amd import SparseFactorizationMachineRanker

    X, Z, train, held = planted_problem()
    kw = dict(E2E_KW, batch_size=1, max_iter=2)
    new = dict(margin=1.0, proposal=None, proposal_power=0.75, sample_weight=None)
    for route in (dict(), dict(sampler="dynamic", n_candidates=4, exclude=held)):
        fits = []
        for extra in ({}, new):
            est = SparseFactorizationMachineRanker(**kw)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                est.fit(X, Z, interactions=train, n_negatives=2, **route, **extra)
            fits.append(est)
        assert np.array_equal(fits[0].P_, fits[1].P_) and np.array_equal(fits[0].w_, fits[1].w_)
        assert fits[0].it_ == fits[1].it_ == 1 + 2 * 1600
    est = SparseFactorizationMachineRanker(**kw)
    with pytest.raises(ValueError, match="objective='pairwise'"):
        est.fit(X, Z, interactions=train, sampler="warp", objective="softmax")
    with pytest.raises(ValueError, match="not to sampler='host'"):
        est.fit(X, Z, interactions=train, proposal="popularity")
    with pytest.raises(ValueError, match="sample_weight"):
        est.fit(X, Z, interactions=train, sampler="warp", sample_weight=np.ones(3))
    with pytest.raises(ValueError, match="proposal"):
        est.fit(X, Z, interactions=train, sampler="warp", proposal=np.zeros(train.shape[1]))
