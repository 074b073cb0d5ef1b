"""Per-feature AdaGrad steps of the minibatch solver on the device: the
raw engine against a reference built from the pinned oracle, graph replay against eager launches,
the accumulator round trip, the refusals behind the C ABI and ``learning_rate='adagrad'`` on the
estimators.  Needs a real MI355X: ``pytest -m gpu``.

The reference: for every minibatch the oracle's ``psgd_epoch`` runs over that minibatch alone on a
copy of the current parameters with rate ``constant``, ``eta0 = 1``, no penalties and
``batch_size = B``, so that ``P_before - P_after`` is the mean gradient; the rule itself is the
dozen NumPy lines of ``_rule``.  Tolerances are those of tests/test_hip_psgd.py for this unit (f64
atomics inside a minibatch, tree reductions): parameters and accumulators ``atol 1e-10``,
``sum_loss`` ``rtol 1e-11``."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N, D = 300, 37
G0 = 1.0   # the default; the accumulated squares below reach several times that
HP = dict(alpha=1e-2, beta=1e-2, eta0=0.05, lr="constant", power_t=0.8)


def _problem():
    """the recipe of test_midsize_against_oracle at n = 300, d = 37, 6 entries per row"""
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(N, D, 6, seed=5)
    X = sp.csr_matrix(X)
    X.data[:] = np.round(X.data * 64) / 64
    lil = X.tolil()
    lil[7, :] = 0        # an empty row
    X = sp.csr_matrix(lil)
    X.eliminate_zeros()
    return X, y


def _start(k, n_orders, seed=1):
    rng = np.random.RandomState(seed)
    P0 = 0.3 * rng.randn(n_orders, k, D)   # gradients large enough to move the steps
    lams = np.sign(rng.randn(k))
    w0 = 0.01 * rng.randn(D)
    return rng, P0, w0, lams


def _eta(lr, eta0, power_t, it):
    return eta0 if lr == "constant" else eta0 / float(it) ** power_t   # 'invscaling'


def _rule(P, w, gP, gw, A_P, A_w, eta, G, alpha, beta, gamma, reg):
    """the specification, on P (n_orders, d, k); accumulators updated in place"""
    A_w += gw ** 2
    ew = eta / np.sqrt(G + A_w)
    w = (w - ew * gw) / (1 + ew * alpha)
    A_P += (gP ** 2).sum(axis=2)
    e = eta / np.sqrt(G + A_P)
    P = (P - e[..., None] * gP) / (1 + e[..., None] * beta)
    c = gamma * e / (1 + e * beta)
    if reg == "l1":
        P = np.sign(P) * np.maximum(np.abs(P) - c[..., None], 0)
    else:
        nr = np.sqrt((P ** 2).sum(axis=2))
        nr = np.where(nr <= c, np.inf, nr)
        P = P * (1 - c / nr)[..., None]
    return P, w


class Reference(object):
    """the state of the rule over epochs of minibatches, gradients from the oracle"""

    def __init__(self, oracle, X, y, P0, w0, lams, degree, reg, G=G0, acc=None):
        self.o, self.X, self.y, self.lams, self.degree, self.reg, self.G = \
            oracle, X, y, lams, degree, reg, G
        self.P = np.ascontiguousarray(P0.swapaxes(1, 2))
        self.w = w0.copy()
        self.A_P = np.zeros(self.P.shape[:2]) if acc is None else acc[0].copy()
        self.A_w = np.zeros(D) if acc is None else acc[1].copy()
        self.it = 1

    def epoch(self, idx, batch, gamma, alpha, beta, eta0, lr, power_t):
        sum_loss = 0.0
        for pos in range(0, idx.size, batch):
            rows = idx[pos:pos + batch]
            B = rows.size
            Pc, wc = self.P.copy(), self.w.copy()
            sl, _ = self.o.psgd_epoch(Pc, wc, self.o.CSR(self.X[rows]), self.y[rows], self.lams,
                                      self.degree, 0.0, 0.0, 0.0, self.reg, "squared",
                                      np.arange(B, dtype=np.int32), True, 1.0, "constant", 1.0,
                                      B, 1)
            sum_loss += sl
            self.P, self.w = _rule(self.P, self.w, self.P - Pc, self.w - wc, self.A_P, self.A_w,
                                   _eta(lr, eta0, power_t, self.it), self.G, alpha, beta, gamma,
                                   self.reg)
            self.it += 1
        return sum_loss

    def P_kd(self):
        return self.P.swapaxes(1, 2)


def _engine(X, y, P0, w0, lams, reg, degree):
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "squared", reg, degree)
    return eng


def _state(eng, P0):
    Pd, wd = np.empty_like(P0), np.empty(D)
    eng.get_params(Pd, wd)
    return (Pd, wd) + eng.psgd_get_adaptive()


def _assert_state(eng, ref, P0, atol=1e-10):
    Pd, wd, aP, aw = _state(eng, P0)
    np.testing.assert_allclose(Pd, ref.P_kd(), rtol=0, atol=atol)
    np.testing.assert_allclose(wd, ref.w, rtol=0, atol=atol)
    np.testing.assert_allclose(aP, ref.A_P, rtol=0, atol=atol)
    np.testing.assert_allclose(aw, ref.A_w, rtol=0, atol=atol)
    return Pd


GAMMA = {"l1": 0.2, "l21": 1.5}


@pytest.mark.parametrize("reg,k,degree,n_orders,batch,gamma", [
    ("l1", 12, 2, 1, 16, GAMMA["l1"]), ("l21", 30, 2, 1, 50, GAMMA["l21"]),
    ("l1", 64, 3, 2, 7, GAMMA["l1"]), ("l21", 70, 3, 2, 64, GAMMA["l21"]),
    ("l1", 130, 4, 3, 300, GAMMA["l1"]), ("l21", 16, 2, 1, 1, 0.2),
    ("l1", 12, 2, 1, 16, 0.0),
])
def test_two_epochs_against_oracle_rule(oracle, reg, k, degree, n_orders, batch, gamma):
    """Every lane width (16/32/64), k > 64 chunking (l21's norm and the accumulator's sum cross
    chunks), several orders, a ragged last batch, B = 1, d no multiple of the groups per block;
    two epochs of a shuffled order."""
    X, y = _problem()
    rng, P0, w0, lams = _start(k, n_orders)
    eng = _engine(X, y, P0, w0, lams, reg, degree)
    eng.psgd_set_adaptive(1, G0)
    ref = Reference(oracle, X, y, P0, w0, lams, degree, reg)
    it = 1
    for ep in range(2):
        idx = rng.permutation(N).astype(np.int32)
        sl_d, it = eng.psgd_epoch(degree, HP["alpha"], HP["beta"], gamma, HP["eta0"], HP["lr"],
                                  HP["power_t"], batch, idx, True, it)
        sl_r = ref.epoch(idx, batch, gamma, **HP)
        print("epoch", ep, "sum_loss", sl_d, sl_r)
        assert it == ref.it
        np.testing.assert_allclose(sl_d, sl_r, rtol=1e-11)
    Pd = _assert_state(eng, ref, P0)
    eng.close()
    # the steps really differ per feature: the accumulators are not small against G0
    assert ref.A_P.max() > G0 and ref.A_P.max() > 3 * ref.A_P.min()
    if reg == "l1":
        nz = np.mean(Pd != 0)
        print("non-zero share", nz)
        if batch == 16 and gamma > 0:      # enough updates for the prox to bite
            assert 0.02 < nz < 0.98, nz    # ... it really prunes and really keeps
        assert np.array_equal(Pd == 0, ref.P_kd() == 0)


def test_graph_replay_equals_eager_with_changing_scalars(oracle):
    """Three epochs of 75 minibatches (two cached runs of 32 replayed per epoch) on one handle per
    route; eta0, beta and gamma change before the third epoch: a recorded graph must not hold
    any of them."""
    reg, k, degree, batch = "l1", 12, 2, 4
    X, y = _problem()
    rng, P0, w0, lams = _start(k, 1)
    orders = [rng.permutation(N).astype(np.int32) for _ in range(3)]
    steps = [dict(HP, gamma=0.04), dict(HP, gamma=0.04),
             dict(HP, gamma=0.09, eta0=0.02, beta=0.3)]
    G = 0.5
    ref = Reference(oracle, X, y, P0, w0, lams, degree, reg, G=G)
    sl_ref = [ref.epoch(idx, batch, **hp) for idx, hp in zip(orders, steps)]
    assert 0.02 < np.mean(ref.P != 0) < 0.98
    got = []
    for eager in (0, 1):
        eng = _engine(X, y, P0, w0, lams, reg, degree)
        eng.set_option("psgd_eager", eager)
        eng.psgd_set_adaptive(1, G)
        it = 1
        for idx, hp, sl_r in zip(orders, steps, sl_ref):
            sl_d, it = eng.psgd_epoch(degree, hp["alpha"], hp["beta"], hp["gamma"], hp["eta0"],
                                      hp["lr"], hp["power_t"], batch, idx, True, it)
            np.testing.assert_allclose(sl_d, sl_r, rtol=1e-9)
        assert it == ref.it
        _assert_state(eng, ref, P0, atol=1e-9)
        got.append(_state(eng, P0))
        eng.close()
    for a, b in zip(*got):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-9)


def test_base_rate_invscaling(oracle):
    """the entry's learning_rate gives the base rate, tabulated per minibatch"""
    reg, k, degree, batch = "l21", 12, 2, 16
    X, y = _problem()
    rng, P0, w0, lams = _start(k, 1)
    hp = dict(HP, lr="invscaling", power_t=0.5, eta0=0.2)
    ref = Reference(oracle, X, y, P0, w0, lams, degree, reg)
    flat = Reference(oracle, X, y, P0, w0, lams, degree, reg)
    eng = _engine(X, y, P0, w0, lams, reg, degree)
    eng.psgd_set_adaptive(1, G0)
    it = 1
    for ep in range(2):
        idx = rng.permutation(N).astype(np.int32)
        sl_d, it = eng.psgd_epoch(degree, hp["alpha"], hp["beta"], GAMMA[reg], hp["eta0"],
                                  hp["lr"], hp["power_t"], batch, idx, True, it)
        np.testing.assert_allclose(sl_d, ref.epoch(idx, batch, GAMMA[reg], **hp), rtol=1e-11)
        flat.epoch(idx, batch, GAMMA[reg], **dict(hp, lr="constant"))
    _assert_state(eng, ref, P0)
    eng.close()
    assert np.abs(ref.P - flat.P).max() > 1e-4   # the case tells the two base rules apart


def test_accumulator_round_trip(oracle):
    reg, k, degree, batch = "l1", 12, 2, 16
    X, y = _problem()
    rng, P0, w0, lams = _start(k, 1)
    idx = [rng.permutation(N).astype(np.int32) for _ in range(2)]
    args = (degree, HP["alpha"], HP["beta"], GAMMA[reg], HP["eta0"], HP["lr"], HP["power_t"],
            batch)
    a = _engine(X, y, P0, w0, lams, reg, degree)
    a.psgd_set_adaptive(1, G0)
    _, it = a.psgd_epoch(*args, idx[0], True, 1)
    P1, w1, aP, aw = _state(a, P0)
    assert aP.shape == (1, D) and aw.shape == (D,) and aP.min() >= 0 and aP.max() > 0
    b = _engine(X, y, P1, w1, lams, reg, degree)
    b.psgd_set_adaptive(1, G0, aP, aw)
    for got, want in zip(b.psgd_get_adaptive(), (aP, aw)):
        assert np.array_equal(got, want)
    sl_a, _ = a.psgd_epoch(*args, idx[1], True, it)
    sl_b, _ = b.psgd_epoch(*args, idx[1], True, it)
    np.testing.assert_allclose(sl_a, sl_b, rtol=1e-12)
    for x, z in zip(_state(a, P0), _state(b, P0)):
        np.testing.assert_allclose(x, z, rtol=0, atol=1e-12)
    # NULL pointers zero the accumulators
    a.psgd_set_adaptive(1, G0)
    assert all(not v.any() for v in a.psgd_get_adaptive())
    # ... and from zero the next epoch is the reference's first epoch from these parameters
    P2, w2, _, _ = _state(a, P0)
    ref = Reference(oracle, X, y, P2, w2, lams, degree, reg)
    ref.it = 5
    a.psgd_epoch(*args, idx[0], True, 5)
    ref.epoch(idx[0], batch, GAMMA[reg], **HP)
    _assert_state(a, ref, P0)
    a.close()
    b.close()


def test_refusals_behind_the_c_abi():
    from sparsepoly_amd.engine import HipEngine

    X, y = _problem()
    rng, P0, w0, lams = _start(12, 1)
    idx = np.arange(N, dtype=np.int32)
    args = (2, HP["alpha"], HP["beta"], 0.2, HP["eta0"], "constant", 1.0, 16, idx, True, 1)
    eng = HipEngine(0, "f64")
    eng.set_data(X, y)
    eng.n_orders, eng.k, eng.d = 1, 12, D
    with pytest.raises(ValueError, match="set_adaptive: set the parameters first"):
        eng.psgd_set_adaptive(1, 1.0)
    with pytest.raises(ValueError, match="get_adaptive"):
        eng.psgd_get_adaptive()
    eng.set_params(P0, w0, lams)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="initial_accumulator must be positive and finite"):
            eng.psgd_set_adaptive(1, bad)
    with pytest.raises(ValueError, match="mode must be 0"):
        eng.psgd_set_adaptive(2, 1.0)
    with pytest.raises(ValueError, match="acc_P holds a negative"):
        eng.psgd_set_adaptive(1, 1.0, -np.ones((1, D)), None)
    for reg in ("squaredl12", "squaredl21"):
        eng.configure("psgd", "squared", reg, 2)
        eng.psgd_set_adaptive(1, 1.0)
        with pytest.raises(ValueError, match="psgd: adaptive steps cannot be combined with "
                                             "squaredl12 / squaredl21"):
            eng.psgd_epoch(*args)
        Pd, wd = np.empty_like(P0), np.empty(D)
        eng.get_params(Pd, wd)
        assert np.array_equal(Pd, P0) and np.array_equal(wd, w0)
        assert all(not v.any() for v in eng.psgd_get_adaptive())
    # the learning_rate codes of the entries are what they were
    eng.configure("psgd", "squared", "l1", 2)
    with pytest.raises(ValueError, match="learning_rate is not supported"):
        eng.psgd_epoch(*(args[:5] + (4,) + args[6:]))
    # parameters of another shape: the accumulators no longer fit
    eng.set_params(np.concatenate([P0, P0]), w0, lams)
    eng.configure("psgd", "squared", "l1", 3)
    with pytest.raises(ValueError, match="accumulators do not fit the parameters"):
        eng.psgd_epoch(*((3,) + args[1:]))
    eng.close()


def test_mode_off_is_the_plain_epoch_bit_for_bit():
    X, y = _problem()
    rng, P0, w0, lams = _start(12, 1)
    idx = rng.permutation(N).astype(np.int32)
    args = (2, HP["alpha"], HP["beta"], 0.04, HP["eta0"], "optimal", 0.8, 4, idx, True, 1)
    out = []
    for touch in (False, True):
        eng = _engine(X, y, P0, w0, lams, "l1", 2)
        if touch:
            eng.psgd_set_adaptive(1, G0)
            eng.psgd_set_adaptive(0, G0)
        sl, it = eng.psgd_epoch(*args)
        Pd, wd = np.empty_like(P0), np.empty(D)
        eng.get_params(Pd, wd)
        out.append((np.array([sl, it]), Pd, wd))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _fit(est, X, y):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return est.fit(X, y)


@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_estimators_warm_start_continues_the_fit(kind):
    """max_iter=2 equals max_iter=1 followed by a warm start of one more epoch: it_ and the
    accumulators are uploaded again"""
    from sparsepoly_amd import (SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)

    X, y = _problem()
    kw = dict(degree=3, n_components=5, solver="psgd", regularizer="l1", alpha=1e-2, beta=1e-2,
              gamma=1e-3, eta0=0.05, learning_rate="adagrad", shuffle=False, batch_size=16,
              tol=-1.0, n_iter_no_change=1000, random_state=0, precision="f64")
    if kind == "regressor":
        cls = SparseFactorizationMachineRegressor
    else:
        cls, y = SparseFactorizationMachineClassifier, np.where(y > np.median(y), 1.0, -1.0)
        kw["loss"] = "logistic"
    assert "adagrad_init" not in cls().get_params() and cls.adagrad_init == 1.0
    two = _fit(cls(max_iter=2, **kw), X, y)
    one = _fit(cls(max_iter=1, warm_start=True, **kw), X, y)
    assert one.adagrad_P_.shape == (2, D) and one.adagrad_w_.shape == (D,)
    assert one.adagrad_P_.max() > 0 and one.adagrad_w_.max() > 0
    _fit(one, X, y)
    one.release_device()
    assert one.it_ == two.it_
    for name in ("P_", "w_", "adagrad_P_", "adagrad_w_"):
        np.testing.assert_allclose(getattr(one, name), getattr(two, name), rtol=0, atol=1e-10,
                                   err_msg=name)
    assert 0 < np.mean(two.P_ != 0) and np.abs(two.P_).max() > 1e-3
    # G0 is the class attribute; with a small one the steps are far from the constant rule's
    class Small(cls):
        adagrad_init = 0.01

    small = _fit(Small(max_iter=2, **kw), X, y)
    flat = _fit(cls(max_iter=2, **dict(kw, learning_rate="constant")), X, y)
    assert not hasattr(flat, "adagrad_P_")
    assert np.abs(small.w_ - two.w_).max() > 1e-5 and np.abs(small.w_ - flat.w_).max() > 1e-5


def test_estimator_refusals():
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    X, y = _problem()
    kw = dict(solver="psgd", learning_rate="adagrad", max_iter=1)
    with pytest.raises(ValueError, match="squaredl12 / squaredl21"):
        SparseFactorizationMachineRegressor(regularizer="squaredl12", **kw).fit(X, y)
    with pytest.raises(ValueError, match="one GPU"):
        SparseFactorizationMachineRegressor(regularizer="l1", distributed=True, **kw).fit(X, y)
