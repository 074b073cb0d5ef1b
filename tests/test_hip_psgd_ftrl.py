"""FTRL-Proximal steps on the device against the float64 rule fed with the
oracle's gradients, as tests/test_hip_psgd_adagrad.py does and at its bar.  ``pytest -m gpu``."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N, D = 60, 40
NEVER, ONCE, ZERO = 11, 23, 5   # stored by no row | by row 0 alone | P0 = 0 and small gradients
G0, HP = 0.8, dict(alpha=1e-2, beta=3e-2, eta0=0.05)
GAMMA = {"l1": 1.5, "l21": 40.0}   # above what reaches z of column ZERO in two epochs


def _problem():
    from sparsepoly_amd.synth import make_problem
    X, y = make_problem(N, D, 5, seed=5)
    lil = sp.lil_matrix(X)
    lil[:, [NEVER, ONCE]] = 0
    lil[0, ONCE] = 0.75
    lil[:, ZERO] *= 0.125
    lil[7, :] = 0        # an empty row: with batch = 1 a minibatch that touches nothing
    X = sp.csr_matrix(lil)
    X.data[:] = np.round(X.data * 64) / 64   # exact in f32 storage, like y
    X.eliminate_zeros()
    return X, np.round(y * 64) / 64


def _start(k, n_orders):
    rng = np.random.RandomState(1)
    P0 = 0.3 * rng.randn(n_orders, k, D)
    P0[:, :, ZERO] = 0.0
    return P0, 0.01 * rng.randn(D), np.sign(rng.randn(k))


def _closed(z, n, eta, pen, gamma, reg):
    den = ((G0 + np.sqrt(n)) / eta + pen)[..., None]
    if reg == "l1":
        return -np.sign(z) * np.maximum(np.abs(z) - gamma, 0) / den
    nr = np.sqrt((z ** 2).sum(axis=-1, keepdims=True))
    keep = np.where(nr > gamma, 1 - gamma / np.where(nr > 0, nr, 1), 0) if reg else 1.0
    return -keep * z / den


class Reference(object):
    """the rule over epochs of minibatches on P (n_orders, d, k), gradients from the oracle;
    ``hp``: what the setter derives the starting state with (``state`` None), ``it``: the number
    of the first minibatch"""

    def __init__(self, oracle, X, y, P0, w0, lams, degree, reg, gamma, loss="squared",
                 fit_linear=True, hp=HP, it=1, state=None):
        from sparsepoly_amd.pairwise import ftrl_start   # (pinned by test_psgd_ftrl_host.py)

        self.o, self.X, self.y, self.lams, self.degree, self.reg = oracle, X, y, lams, degree, reg
        self.loss, self.fit_linear = loss, fit_linear
        self.P, self.w, self.it = np.ascontiguousarray(P0.swapaxes(1, 2)), w0.copy(), it
        if state is None:
            state = ftrl_start(P0, w0, G0, hp["eta0"], hp["alpha"], hp["beta"], gamma, reg)
        z, zw, n, nw = (np.array(a, dtype=np.double) for a in state)
        self.z, self.zw, self.n, self.nw = np.ascontiguousarray(z.swapaxes(1, 2)), zw, n, nw

    def epoch(self, idx, batch, gamma, alpha, beta, eta0, learning_rate="constant", power_t=1.0):
        """-> the sum of the rows' losses; minibatch number ``it`` steps with the rates
        ``_psgd_eta`` tabulates for it: ``eta_P`` in P's sigma and denominator, ``eta_w`` in w's"""
        from sparsepoly_amd.pairwise import _psgd_eta

        sum_loss = 0.0
        for pos in range(0, idx.size, batch):
            rows = idx[pos:pos + batch]
            Pc, wc = self.P.copy(), self.w.copy()
            sl, _ = self.o.psgd_epoch(Pc, wc, self.o.CSR(self.X[rows]), self.y[rows], self.lams,
                                      self.degree, 0.0, 0.0, 0.0, self.reg, self.loss,
                                      np.arange(rows.size, dtype=np.int32), self.fit_linear, 1.0,
                                      "constant", 1.0, rows.size, 1)
            sum_loss += sl
            eta_P, eta_w = _psgd_eta(learning_rate, eta0, alpha, beta, power_t, self.it)
            for p, z, n, pen, r, eta in (
                    (self.P, self.z, self.n, beta, self.reg, eta_P),
                    (self.w[:, None], self.zw[:, None], self.nw, alpha, None, eta_w)):
                g = p - (Pc if r else wc[:, None])   # (fit_linear off: the oracle leaves w, g = 0)
                g2 = (g ** 2).sum(axis=-1)
                z += g - ((np.sqrt(n + g2) - np.sqrt(n)) / eta)[..., None] * p
                n += g2
                p[...] = np.where((g2 != 0)[..., None], _closed(z, n, eta, pen, gamma, r), p)
            self.it += 1
        return sum_loss

    def state(self):
        return (self.P.swapaxes(1, 2), self.w, self.z.swapaxes(1, 2), self.zw, self.n, self.nw)


def _engine(X, y, P0, w0, lams, reg, degree, gamma, precision="f64", state=None, mode=1):
    from sparsepoly_amd.engine import HipEngine
    eng = HipEngine(0, precision)
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "squared", reg, degree)
    if mode is not None:   # (None: a handle that never sees the setter)
        eng.psgd_set_ftrl(mode, G0, HP["eta0"], HP["alpha"], HP["beta"], gamma, state)
    return eng


def _state(eng):
    return tuple(eng.get_params()) + eng.psgd_get_ftrl()


def _epoch(eng, degree, gamma, batch, idx, it, hp=HP, **kw):
    return eng.psgd_epoch(degree, hp["alpha"], hp["beta"], gamma, hp["eta0"], "constant", 1.0,
                          batch, idx, True, it, **kw)[1]


@pytest.mark.parametrize("reg,k,degree,n_orders,batch,precision", [
    ("l1", 8, 2, 1, 7, "f64"), ("l21", 30, 3, 2, 1, "f32"), ("l1", 64, 3, 1, N, "f32"),
    ("l21", 70, 2, 1, 7, "f64"), ("l1", 70, 3, 2, 1, "f64"), ("l21", 8, 3, 2, N, "f32"),
    ("l21", 64, 2, 1, 1, "f64"), ("l1", 30, 2, 1, N, "f64"),
])
def test_two_epochs_against_the_oracle_rule(oracle, reg, k, degree, n_orders, batch, precision):
    X, y = _problem()
    P0, w0, lams = _start(k, n_orders)
    gamma = GAMMA[reg]
    eng = _engine(X, y, P0, w0, lams, reg, degree, gamma, precision)
    ref = Reference(oracle, X, y, P0, w0, lams, degree, reg, gamma)
    first = _state(eng)
    rng, it = np.random.RandomState(2), 1
    for ep in range(2):
        idx = rng.permutation(N).astype(np.int32)
        it = _epoch(eng, degree, gamma, batch, idx, it)
        ref.epoch(idx, batch, gamma, **HP)
    got = _state(eng)
    assert it == ref.it
    for a, b in zip(got, ref.state()):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10)
    P, n = ref.P, ref.n   # ZERO: reached by gradients, zeroed by the threshold; the others survive
    assert (n[:, ZERO] > 0).all() and not P[:, ZERO].any() and ref.z[:, ZERO].all(axis=1).all()
    assert n[:, ONCE].all() and (np.abs(P).max(axis=2) > 0).sum(axis=1).min() >= D - 2
    assert np.array_equal(got[0] == 0, ref.state()[0] == 0)
    assert first[0][..., NEVER].any() and first[2][..., NEVER].any()
    for a, b in zip(got, first):
        assert np.array_equal(a[..., NEVER], b[..., NEVER])


def test_a_column_touched_once_stays_what_that_minibatch_made_it():
    """what the first minibatch (rows 0..6, alone on a handle of its own) makes of column ONCE"""
    X, y = _problem()
    P0, w0, lams = _start(30, 2)
    idx = np.arange(N, dtype=np.int32)
    out = []
    for rows in (7, N):
        eng = _engine(X[:rows], y[:rows], P0, w0, lams, "l21", 3, GAMMA["l21"])
        _epoch(eng, 3, GAMMA["l21"], 7, idx[:rows], 1)
        out.append([a[..., ONCE] for a in _state(eng)])
        eng.close()
    assert out[0][4].all() and not np.array_equal(out[0][0], P0[..., ONCE])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_graph_replay_equals_eager_bit_for_bit_with_changing_scalars():
    """batch = 1 (one order of the atomics): a recorded run of 32 minibatches and 28 behind it"""
    X, y = _problem()
    P0, w0, lams = _start(8, 1)
    steps = [(0.3, HP), (0.3, HP), (0.5, dict(HP, eta0=0.02, beta=0.3))]
    rng = np.random.RandomState(4)
    orders = [rng.permutation(N).astype(np.int32) for _ in steps]
    got = []
    for eager in (0, 1):
        eng = _engine(X, y, P0, w0, lams, "l1", 2, 0.3)
        eng.set_option("psgd_eager", eager)
        it = 1
        for idx, (gamma, hp) in zip(orders, steps):
            it = _epoch(eng, 2, gamma, 1, idx, it, hp)
        got.append(_state(eng))
        eng.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)


def test_state_round_trip_and_mode_off():
    X, y = _problem()
    P0, w0, lams = _start(8, 1)
    idx = np.arange(N, dtype=np.int32)
    a = _engine(X, y, P0, w0, lams, "l1", 2, 0.3)
    it = _epoch(a, 2, 0.3, 1, idx, 1)
    mid = _state(a)
    b = _engine(X, y, mid[0], mid[1], lams, "l1", 2, 0.3, state=mid[2:])
    assert a.psgd_ftrl_mode() == (1, G0)
    for eng in (a, b):
        _epoch(eng, 2, 0.3, 1, idx[::-1].copy(), it)
    for u, v in zip(_state(a), _state(b)):
        assert np.array_equal(u, v)
    outs = []   # mode off: the plain epoch, bit for bit that of a handle without the setter
    for mode in (0, None):
        eng = _engine(X, y, P0, w0, lams, "l1", 2, 0.3, mode=mode)
        _epoch(eng, 2, 0.3, 7, idx, 1)
        outs.append(eng.get_params())
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_refusals_leave_the_parameters_alone():
    X, y = _problem()
    P0, w0, lams = _start(8, 1)
    idx = np.arange(N, dtype=np.int32)
    eng = _engine(X, y, P0, w0, lams, "l1", 2, 0.3)
    for bad, msg in (((2, G0, 0.05), "mode must be 0"), ((1, 0.0, 0.05), "G0 must be positive"),
                     ((1, G0, -1.0), "eta0 must be positive")):
        with pytest.raises(ValueError, match=msg):
            eng.psgd_set_ftrl(*bad)

    def refused(msg, degree=2, **kw):
        before = eng.get_params()
        with pytest.raises(ValueError, match=msg):
            _epoch(eng, degree, 0.3, 7, idx, 1, **kw)
        for u, v in zip(before, eng.get_params()):
            assert np.array_equal(u, v)

    eng.psgd_set_adaptive(1, 1.0)
    refused("ftrl steps and adaptive steps are both")
    eng.psgd_set_adaptive(0, 1.0)
    for reg in ("squaredl12", "squaredl21"):
        eng.configure("psgd", "squared", reg, 2)
        refused("ftrl steps cannot be combined with squaredl12 / squaredl21")
    eng.set_params(np.concatenate([P0, P0]), w0, lams)     # n_orders changed
    eng.configure("psgd", "squared", "l1", 3)
    refused("ftrl state does not fit the parameters", 3)
    eng.set_params(np.concatenate([P0, P0], axis=1), w0, np.concatenate([lams, lams]))  # k changed
    eng.configure("psgd", "squared", "l1", 2)
    refused("ftrl state does not fit the parameters")
    eng.set_data(sp.hstack([X, sp.csr_matrix((N, 3))], format="csr"), y)        # d alone changed
    eng.set_params(np.pad(P0, ((0, 0), (0, 0), (0, 3))), np.pad(w0, (0, 3)), lams)
    eng.configure("psgd", "squared", "l1", 2)
    refused("ftrl state does not fit the parameters")
    eng.set_data(X, y)
    eng.set_params(P0, w0, lams)
    eng.configure("psgd", "squared", "l1", 2)
    eng.psgd_set_ftrl(1, G0, 0.05)
    eng.comm_init(eng.comm_unique_id(), 1, 0)                     # a communicator: several ranks
    refused("ftrl steps are not supported with several ranks", row_lo=0)   # the sharded entry
    eng.close()


NAMES = ("P_", "w_", "ftrl_z_P_", "ftrl_z_w_", "ftrl_n_P_", "ftrl_n_w_")


def test_ranker_softmax_with_uniform_negatives_against_the_restatement():
    from sklearn.utils import check_random_state

    from sparsepoly_amd import SparseFactorizationMachineRanker
    from sparsepoly_amd.pairwise import restate_list_epoch, restate_sample
    from test_hip_pairwise_list import FIT_KW, _fit_problem
    X, Z, I = _fit_problem()
    kw = dict(FIT_KW, learning_rate="ftrl", gamma=1e-3, eta0=0.1, max_iter=2)
    est = SparseFactorizationMachineRanker(**kw).fit(
        X, Z, interactions=I, n_negatives=3, sampler="uniform", objective="softmax", resample=True)
    d, Q = X.shape[1], I.nnz
    rng = check_random_state(kw["random_state"])
    P, w, lams, it, state = 0.01 * rng.randn(1, 6, d), np.zeros(d), np.ones(6), 1, None
    seed = rng.randint(0, 2 ** 31 - 1)
    for ep in range(2):
        t, _, _ = restate_sample(P, w, lams, X, Z, I, 2, 3, 1, 64, seed, ep)
        t = t.reshape(Q, 3, 3)[rng.permutation(Q)].reshape(-1, 3)
        P, w, _, it, state = restate_list_epoch(
            P, w, lams, X, Z, t, 3, 2, "softmax", "logistic", "l1", 1e-3, 1e-2, 1e-3, 0.1,
            "constant", 1.0, 8, True, it, ftrl=est.ftrl_init, state=state)
    assert est.it_ == it
    for name, b in zip(NAMES, (P, w) + state):   # the list tests' bar, two epochs
        np.testing.assert_allclose(getattr(est, name), b, rtol=0, atol=2e-9, err_msg=name)


def test_estimator_warm_start_and_deterministic_fits():
    from sparsepoly_amd import SparseFactorizationMachineRegressor as Reg
    X, y = _problem()
    kw = dict(degree=3, n_components=5, solver="psgd", regularizer="l1", alpha=1e-2, beta=1e-2,
              gamma=0.05, eta0=0.05, learning_rate="ftrl", shuffle=False, batch_size=1,
              tol=-1.0, n_iter_no_change=1000, random_state=0, precision="f64")
    two = Reg(max_iter=2, **kw).fit(X, y)
    one = Reg(max_iter=1, warm_start=True, **kw).fit(X, y).fit(X, y)
    for name in NAMES + ("it_",):   # batch_size = 1: one order of summation, so to the same bits
        assert np.array_equal(getattr(one, name), getattr(two, name)), name

    class Det(Reg):
        deterministic = True

    fits = [Det(max_iter=2, **dict(kw, shuffle=True, batch_size=7)).fit(X, y) for _ in (0, 1)]
    for name in NAMES:
        assert np.array_equal(getattr(fits[0], name), getattr(fits[1], name)), name
