"""The three update rules of the minibatch unit -- plain (``psgd_update_kernel`` and the Michelot
passes), AdaGrad and FTRL-Proximal (19g) -- where no other test takes
them: the third and fourth component chunk (``k`` = 129 .. 256, ``kPsgdMaxC = 4``) and the second
trip of the grid-stride loops of the dense passes (``d`` beyond ``kPsgdNB`` workgroups of
``kBlock / L`` columns; beyond ``kPsgdNB * kBlock`` columns for the one-thread-per-column ``w``
loop).  Each rule against the oracle the way its own test file does it and at that file's bars
(tests/test_hip_psgd.py, test_hip_psgd_adagrad.py, test_hip_psgd_ftrl.py: parameters and state
``atol 1e-10``, ``sum_loss`` ``rtol 1e-11``).  The references are computed on the host by
tests/test_psgd_update_shapes_host.py, which also shows that they mean something.
``pytest -m gpu``."""
import numpy as np
import pytest

import test_psgd_update_shapes_host as H

pytestmark = pytest.mark.gpu

ATOL, LOSS_RTOL = 1e-10, 1e-11
NAMES = {"plain": ("P", "w"), "adagrad": ("P", "w", "A_P", "A_w"),
         "ftrl": ("P", "w", "z_P", "z_w", "n_P", "n_w")}


def _engine(rule, reg, X, y, P0, w0, lams, degree=2, det=0):
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "squared", reg, degree)
    if rule == "adagrad":
        eng.psgd_set_adaptive(1, H.ADA_G0)
    elif rule == "ftrl":
        eng.psgd_set_ftrl(1, H.G0, H.fr.HP["eta0"], H.fr.HP["alpha"], H.fr.HP["beta"],
                          H.FTRL_GAMMA[reg])
    if det:
        eng.psgd_set_deterministic(1)
    return eng


def _step(rule, reg, degree, batch):
    if rule == "plain":
        hp, gamma, lr, power_t = H.PLAIN_HP, H.PLAIN_GAMMA[reg], "optimal", 0.8
    elif rule == "adagrad":
        hp, gamma, lr, power_t = H.ADA_HP, H.ADA_GAMMA[reg], "constant", 0.8
    else:
        hp, gamma, lr, power_t = H.fr.HP, H.FTRL_GAMMA[reg], "constant", 1.0
    return (degree, hp["alpha"], hp["beta"], gamma, hp["eta0"], lr, power_t, batch)


def _arrays(eng, rule):
    out = tuple(eng.get_params())
    if rule == "adagrad":
        out += tuple(eng.psgd_get_adaptive())
    elif rule == "ftrl":
        out += tuple(eng.psgd_get_ftrl())
    return out


def _run(eng, rule, reg, orders, batch, ref, tag):
    """the epochs on ``eng`` (closed here) against ``ref``; -> (arrays before, arrays after)"""
    try:
        first = _arrays(eng, rule)
        it = 1
        for idx, sl_r in zip(orders, ref["loss"]):
            sl, it = eng.psgd_epoch(*_step(rule, reg, 2, batch), idx, True, it)
            print("%s: rel dloss = %.3e" % (tag, abs(sl - sl_r) / abs(sl_r)))
            np.testing.assert_allclose(sl, sl_r, rtol=LOSS_RTOL)
        got = _arrays(eng, rule)
    finally:
        eng.close()
    assert it == ref["it"]
    print(tag + ": " + "  ".join("max|d%s| = %.3e" % (n, np.abs(a - b).max())
                                 for n, a, b in zip(NAMES[rule], got, ref["arrays"])))
    for n, a, b in zip(NAMES[rule], got, ref["arrays"]):
        np.testing.assert_allclose(a, b, rtol=0, atol=ATOL, err_msg=n)
    if reg in ("l1", "squaredl12"):
        assert np.array_equal(got[0] == 0, ref["arrays"][0] == 0)
    return first, got


@pytest.mark.parametrize("rule,reg,k", H.CHUNK_CASES)
def test_component_chunks_three_and_four(rule, reg, k):
    """two epochs of batch 7 (a ragged last minibatch of 4) on 60 x 40 at k = 128 .. 256: the
    first epoch of a squared-norm regularizer runs eagerly, the second replays graphs"""
    X, y, orders = H.chunk_problem()
    P0, w0, lams = H.chunk_start(k)
    ref = H.chunk_reference(rule, reg, k)
    first, got = _run(_engine(rule, reg, X, y, P0, w0, lams), rule, reg, orders, H.CHUNK_BATCH,
                      ref, "%s %s k=%d" % (rule, reg, k))
    if rule == "ftrl":
        for a, b in zip(got, first):
            assert np.array_equal(a[..., H.fr.NEVER], b[..., H.fr.NEVER])


def test_deterministic_gradients_at_the_fourth_chunk():
    """psgd_set_deterministic(1): the fixed-order gradient kernels chunk the components too"""
    X, y, orders = H.chunk_problem()
    P0, w0, lams = H.chunk_start(193)
    ref = H.chunk_reference("plain", "squaredl12", 193)
    outs = []
    for _ in (0, 1):
        eng = _engine("plain", "squaredl12", X, y, P0, w0, lams, det=1)
        outs.append(_run(eng, "plain", "squaredl12", orders, H.CHUNK_BATCH, ref, "det k=193")[1])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_pair_epoch_at_the_fourth_chunk():
    """the pair gradient kernel at k = 193, batch 7 (bars of tests/test_hip_pairwise.py as
    tests/test_hip_psgd_dispatch.py takes them)"""
    from sparsepoly_amd.engine import HipEngine

    pairs = H.pairs
    X, Z, S, y, t, I, order = pairs.problem()
    P0, w0, lams = pairs.params(193)
    Pr, wr, slr, itr = H.chunk_pair_reference()
    ts = (t + np.array([0, pairs.N_CTX, pairs.N_CTX])).astype(np.int32)
    eng = HipEngine(0, "f64")
    try:
        eng.set_data(S, y)
        eng.set_params(P0, w0, lams)
        eng.configure("psgd", "logistic", "l1", pairs.DEGREE)
        hp = pairs.HYPER
        sl, it = eng.psgd_pairs_epoch(pairs.DEGREE, hp["alpha"], hp["beta"], pairs.GAMMA,
                                      hp["eta0"], hp["learning_rate"], hp["power_t"], 7, ts, True,
                                      1)
        P, w = eng.get_params()
    finally:
        eng.close()
    print("pair epoch k=193: max|dP| = %.3e  max|dw| = %.3e  rel dloss = %.3e"
          % (np.abs(P - Pr).max(), np.abs(w - wr).max(), abs(sl - slr) / abs(slr)))
    assert it == itr
    np.testing.assert_allclose(sl, float(slr), rtol=1e-10)
    np.testing.assert_allclose(P, Pr, rtol=0, atol=1e-9)
    np.testing.assert_allclose(w, wr, rtol=0, atol=1e-9)


def test_257_components_are_refused_and_256_run():
    from sparsepoly_amd.engine import HipEngine

    X, y, orders = H.chunk_problem()
    rng = np.random.RandomState(5)
    P257, w257, l257 = 0.05 * rng.randn(1, 257, H.fr.D), 0.01 * rng.randn(H.fr.D), np.ones(257)
    eng = HipEngine(0, "f64")
    try:
        eng.set_data(X, y)
        eng.set_params(P257, w257, l257)
        with pytest.raises(NotImplementedError, match="n_components > 256"):
            eng.configure("psgd", "squared", "l1", 2)
        P, w = eng.get_params()
        assert np.array_equal(P, P257) and np.array_equal(w, w257)
        P0, w0, lams = H.chunk_start(256)
        eng.set_params(P0, w0, lams)
        eng.configure("psgd", "squared", "l1", 2)
    except BaseException:
        eng.close()
        raise
    _run(eng, "plain", "l1", orders, H.CHUNK_BATCH, H.chunk_reference("plain", "l1", 256),
         "after the refusal, k=256")


@pytest.mark.parametrize("rule,reg,k,d", H.STRIDE_CASES)
def test_second_trip_of_the_grid_stride_loops(rule, reg, k, d):
    """one epoch of two minibatches at d just beyond the grid's first trip: stored columns in
    both trips, at the first column of the second and at d - 1"""
    X, y, P0, w0, lams, orders, stored = H.stride_problem(k, d)
    ref = H.stride_reference(rule, reg, k, d)
    first, got = _run(_engine(rule, reg, X, y, P0, w0, lams), rule, reg, orders, H.STRIDE_BATCH,
                      ref, "%s %s k=%d d=%d" % (rule, reg, k, d))
    if rule == "ftrl":   # the never-stored columns keep all their bits, in both trips
        never = np.setdiff1d(np.arange(d), stored)
        for a, b in zip(got, first):
            assert np.array_equal(a[..., never], b[..., never])
        for a, b in zip(got[2:], H.rule_start_state(rule, reg, P0, w0)[2:]):
            np.testing.assert_allclose(a[..., never], b[..., never], rtol=0, atol=ATOL)
