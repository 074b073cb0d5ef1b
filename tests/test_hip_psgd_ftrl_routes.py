"""FTRL-Proximal steps through every gradient route that feeds them,
against the float64 rule: pointwise (atomic and deterministic) with the oracle's gradients, pairs,
weighted pairs, sampled pairs, deterministic pairs and lists with the restatements of
``sparsepoly_amd.pairwise``.  Two epochs, the state carried into the second; rates that differ
between ``P`` and ``w`` and move with every minibatch (``optimal``, ``pegasos``, ``invscaling``);
``fit_linear`` off; columns that revive and die; the lazy branch on stored columns; the state
round trip with two orders and two component chunks.

Bars: pointwise ``atol 1e-10`` on the six arrays (tests/test_hip_psgd_ftrl.py), ``sum_loss``
``rtol 1e-10``; pairs and lists ``atol 2e-9`` and ``rtol 1e-10`` (the FTRL ranker test,
tests/test_hip_pairwise.py).  The references and the proof that they mean something are in
tests/test_psgd_update_shapes_host.py.  ``pytest -m gpu``."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_psgd_update_shapes_host as H

pytestmark = pytest.mark.gpu

pairs, fr = H.pairs, H.fr
NAMES = ("P", "w", "z_P", "z_w", "n_P", "n_w")
SHIFT = np.array([0, pairs.N_CTX, pairs.N_CTX], dtype=np.int32)


def _state(eng):
    return tuple(eng.get_params()) + tuple(eng.psgd_get_ftrl())


def _compare(tag, got, ref, atol, losses, it):
    print(tag + ": " + "  ".join("max|d%s| = %.3e" % (n, np.abs(a - b).max())
                                 for n, a, b in zip(NAMES, got, ref["arrays"])))
    assert it == ref["it"]
    for sl, sl_r in zip(losses, ref["loss"]):
        print("%s: rel dloss = %.3e" % (tag, abs(sl - sl_r) / max(abs(sl_r), 1e-300)))
        np.testing.assert_allclose(sl, sl_r, rtol=1e-10)
    for n, a, b in zip(NAMES, got, ref["arrays"]):
        np.testing.assert_allclose(a, b, rtol=0, atol=atol, err_msg=n)


# ------------------------------------------------------------------ pointwise
def _point_engine(c, X, y, P0, w0, lams, state=None):
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", c["loss"], c["reg"], c["degree"])
    hp = c["hp"]
    eng.psgd_set_ftrl(1, H.G0, hp["eta0"], hp["alpha"], hp["beta"], c["gamma"], state)
    if c["det"]:
        eng.psgd_set_deterministic(1)
    return eng


def _point_epoch(eng, c, idx, it):
    hp = c["hp"]
    return eng.psgd_epoch(c["degree"], hp["alpha"], hp["beta"], c["gamma"], hp["eta0"],
                          hp["learning_rate"], hp["power_t"], c["batch"], idx, c["fit_linear"], it)


def _point_run(name, data=None):
    """the case's two epochs -> (state before, state after, it, losses); ``data``: one matrix per
    epoch to put in the place of the case's before that epoch (the state stays)"""
    c, X, y, P0, w0, lams, orders = H.point_case(name)
    eng = _point_engine(c, X, y, P0, w0, lams)
    try:
        first, it, losses = _state(eng), c["it0"], []
        for ep, idx in enumerate(orders):
            if data is not None:
                eng.set_data(data[ep], y)
                eng.configure("psgd", c["loss"], c["reg"], c["degree"])
            sl, it = _point_epoch(eng, c, idx, it)
            losses.append(sl)
        got = _state(eng)
    finally:
        eng.close()
    return first, got, it, losses


@pytest.mark.parametrize("name", ["optimal-l1", "optimal-l21", "invscaling", "pegasos",
                                  "logistic"])
def test_pointwise_rates_that_differ_and_move(name):
    """eta_P in P's sigma and denominator, eta_w in w's, each minibatch at its own ``it``"""
    first, got, it, losses = _point_run(name)
    _compare(name, got, H.point_reference(name), 1e-10, losses, it)
    for a, b in zip(got, first):   # the never-stored column keeps its bits
        assert np.array_equal(a[..., fr.NEVER], b[..., fr.NEVER])


@pytest.mark.parametrize("name", ["det-l1", "det-l21"])
def test_deterministic_pointwise_against_the_rule(name):
    first, got, it, losses = _point_run(name)
    _compare(name, got, H.point_reference(name), 1e-10, losses, it)
    again = _point_run(name)[1]
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


def test_pointwise_without_the_linear_term():
    first, got, it, losses = _point_run("nolinear")
    _compare("nolinear", got, H.point_reference("nolinear"), 1e-10, losses, it)
    for i in (1, 3, 5):    # w, z_w, n_w: bit for bit their start
        assert np.array_equal(got[i], first[i]), NAMES[i]
    assert first[1].any() and first[3].any()


@pytest.mark.parametrize("name", ["revive-l1", "revive-l21"])
def test_columns_revive_and_die(name):
    """host: a column with P0 = 0 ends non-zero, a live one ends exactly zero; here: the device's
    zero pattern is the reference's"""
    first, got, it, losses = _point_run(name)
    ref = H.point_reference(name)
    _compare(name, got, ref, 1e-10, losses, it)
    assert not first[0][..., fr.ZERO].any()
    assert np.array_equal(got[0] == 0, ref["arrays"][0] == 0)


def test_hinge_rows_past_the_margin_touch_nothing():
    """batch 1, squared hinge: a row past the margin has a gradient of exactly zero on stored
    columns with n > 0.  The same epochs on data in which those rows store nothing -- their
    minibatches taken out of the rule -- leave the same bits."""
    ref = H.point_reference("hinge")
    c, X, y, P0, w0, lams, orders = H.point_case("hinge")
    first, got, it, losses = _point_run("hinge")
    _compare("hinge", got, ref, 1e-10, losses, it)
    data = []
    for idx, past in zip(orders, ref["past"]):
        assert past.size >= 3
        lil = X.tolil()
        lil[idx[past], :] = 0
        data.append(sp.csr_matrix(lil))
    _, cut, it_cut, _ = _point_run("hinge", data)
    assert it_cut == it
    for n, a, b in zip(NAMES, got, cut):
        assert np.array_equal(a, b), n


def test_state_round_trip_two_orders_two_chunks():
    """k = 70, two orders, degree 3: the setter and getter transpose per order; a handle started
    from the downloaded (P, w, state) continues bit for bit (batch 1: one order of the atomics)"""
    c = dict(reg="l1", k=70, degree=3, n_orders=2, batch=1, hp=H.CONSTANT, loss="squared",
             fit_linear=True, det=0, gamma=0.3)
    X, y = fr._problem()
    P0, w0, lams = fr._start(70, 2)
    given = H.round_trip_state()
    idx = np.arange(fr.N, dtype=np.int32)
    a = _point_engine(c, X, y, P0, w0, lams, state=given)
    b = None
    try:
        for n, u, v in zip(NAMES[2:], a.psgd_get_ftrl(), given):
            assert np.array_equal(u, v), n
        a.psgd_set_ftrl(1, H.G0, c["hp"]["eta0"], c["hp"]["alpha"], c["hp"]["beta"], c["gamma"])
        _, it = _point_epoch(a, c, idx, 1)
        mid = _state(a)
        assert (mid[4] > 0).sum(axis=1).min() > fr.D // 2   # both orders touched
        b = _point_engine(c, X, y, mid[0], mid[1], lams, state=mid[2:])
        for u, v in zip(_state(b), mid):
            assert np.array_equal(u, v)
        for eng in (a, b):
            _point_epoch(eng, c, idx[::-1].copy(), it)
        for n, u, v in zip(NAMES, _state(a), _state(b)):
            assert np.array_equal(u, v), n
        assert np.abs(_state(a)[0] - mid[0]).max() > 1e-4
    finally:
        a.close()
        if b is not None:
            b.close()


# ------------------------------------------------------------------ pairs and lists
def _pair_engine(reg, k, hp, det=0, sampler=False):
    from sparsepoly_amd.engine import HipEngine

    X, Z, S, y, t, I, order = pairs.problem()
    P0, w0, lams = pairs.params(k)
    eng = HipEngine(0, "f64")
    eng.set_data(S, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "logistic", reg, pairs.DEGREE)
    eng.psgd_set_ftrl(1, H.G0, hp["eta0"], hp["alpha"], hp["beta"], H.PAIR_GAMMA[reg])
    if det:
        eng.psgd_pairs_set_deterministic(1)
    if sampler:
        eng.psgd_pairs_set_sampler(pairs.N_CTX, pairs.N_CAND, I)
    return eng


def _hyper(reg, hp, batch):
    return (pairs.DEGREE, hp["alpha"], hp["beta"], H.PAIR_GAMMA[reg], hp["eta0"],
            hp["learning_rate"], hp["power_t"], batch)


def _pair_run(route, reg, k, batch, hp=H.OPTIMAL, fit_linear=True, weights=None):
    """two epochs of a route -> (state before, state after, it, losses, reference); the sampled
    route's reference runs on the triples the device reports"""
    t = pairs.problem()[4]
    ts = (t + SHIFT).astype(np.int32)
    step = _hyper(reg, hp, batch)
    eng = _pair_engine(reg, k, hp, det=route == "det", sampler=route == "sampled")
    ref = None
    try:
        first, it, losses = _state(eng), H.IT0, []
        if route == "sampled":
            P, w, _ = pairs.params(k)
            ref, it_r, st = dict(loss=[]), H.IT0, None
        for ep in range(2):
            if route == "weighted":
                sl, it = eng.psgd_pairs_epoch_weighted(*step, ts, weights, fit_linear, it)
            elif route == "sampled":
                m, td, _ = eng.psgd_pairs_sample(pairs.DEGREE, H.SAMPLE["n_neg"], H.SAMPLE["M"],
                                                 H.SAMPLE["max_draws"], H.SAMPLE["seed"], ep)
                assert m == pairs.problem()[5].nnz
                sl, it = eng.psgd_pairs_epoch_sampled(*step, fit_linear, it)
                P, w, sl_r, it_r, st = H.pair_epoch_ref(P, w, st, it_r, td - SHIFT, reg, batch, hp,
                                                        fit_linear)
                ref["loss"].append(float(sl_r))
            else:
                sl, it = eng.psgd_pairs_epoch(*step, ts, fit_linear, it)
            losses.append(sl)
        got = _state(eng)
    finally:
        eng.close()
    if route == "sampled":
        ref.update(arrays=(P, w) + tuple(st), it=it_r)
    return first, got, it, losses, ref


@pytest.mark.parametrize("route,reg,k,batch", H.PAIR_CASES)
def test_pair_routes_against_the_restatement(route, reg, k, batch):
    wt = H.pair_weights() if route == "weighted" else None
    first, got, it, losses, ref = _pair_run(route, reg, k, batch, weights=wt)
    if ref is None:
        ref = H.pair_reference(route, reg, k, batch)
    _compare("%s %s k=%d batch=%d" % (route, reg, k, batch), got, ref, 2e-9, losses, it)
    assert np.abs(got[0] - first[0]).max() > 1e-4
    if route == "det" and batch == 7:   # fixed order: a second handle agrees bit for bit
        again = _pair_run(route, reg, k, batch)[1]
        for n, a, b in zip(NAMES, got, again):
            assert np.array_equal(a, b), n


@pytest.mark.parametrize("hp_name", ["pegasos", "invscaling"])
def test_pair_epoch_under_the_other_schedules(hp_name):
    hp = {"pegasos": H.PEGASOS, "invscaling": H.INVSCALING}[hp_name]
    first, got, it, losses, _ = _pair_run("pairs", "l1", 33, 7, hp)
    _compare("pairs " + hp_name, got, H.pair_reference("pairs", "l1", 33, 7, hp_name), 2e-9,
             losses, it)


def test_pair_epoch_without_the_linear_term():
    first, got, it, losses, _ = _pair_run("pairs", "l21", 16, 7, fit_linear=False)
    _compare("pairs nolinear", got, H.pair_reference("pairs", "l21", 16, 7, "optimal", False),
             2e-9, losses, it)
    for i in (1, 3, 5):
        assert np.array_equal(got[i], first[i]), NAMES[i]


def test_weights_all_zero_touch_nothing():
    """the lazy branch on stored columns: every gradient is exactly zero"""
    first, got, it, losses, _ = _pair_run("weighted", "l1", 70, 7,
                                          weights=np.zeros(pairs.N_TRIPLES))
    assert it == H.IT0 + 2 * 6 and losses == [0.0, 0.0]
    for n, a, b in zip(NAMES, got, first):
        assert np.array_equal(a, b), n
    assert first[0].any() and first[2].any()


@pytest.mark.parametrize("reg,k", [("l1", 33), ("l21", 70)])
def test_list_objective_against_the_restatement(reg, k):
    ts = (H.list_triples() + SHIFT).astype(np.int32)
    eng = _pair_engine(reg, k, H.OPTIMAL)
    try:
        it, losses = H.IT0, []
        for ep in range(2):
            sl, it = eng.psgd_lists_epoch(*_hyper(reg, H.OPTIMAL, H.LIST_BATCH), ts, H.M_LIST,
                                          "list", True, it)
            losses.append(sl)
        got = _state(eng)
    finally:
        eng.close()
    _compare("lists %s k=%d" % (reg, k), got, H.list_reference(reg, k), 2e-9, losses, it)
