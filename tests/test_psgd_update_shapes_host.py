"""The references of tests/test_hip_psgd_ftrl_routes.py and tests/test_hip_psgd_update_shapes.py,
computed on the host (NumPy, the C oracle, the restatements of ``sparsepoly_amd.pairwise``), once
per process (``lru_cache``; treat every array as read-only) and shared with those two modules.
No device is needed here: the tests of this module assert that each device comparison means
something -- the parameters move, touched and untouched columns both exist, the columns of a
grid-stride loop's second trip receive a gradient, the hinge rows past the margin exist, columns
revive and die, the two rates differ, zero and non-zero weights share a minibatch.

The shapes of the stride cases follow from constants of the device headers (``kBlock``,
``kPsgdNB``, ``kPsgdMaxC``, the widths of ``SPFM_DISPATCH_L``); ``test_device_constants`` reads
them there."""
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import test_hip_psgd_dispatch as pairs
import test_hip_psgd_ftrl as fr
from test_hip_psgd_adagrad import _rule as adagrad_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparsepoly_amd", "csrc")
K_BLOCK, K_NB, K_MAXC, WIDTHS = 256, 1024, 4, (16, 32, 64)   # what the shapes below assume

G0 = fr.G0
OPTIMAL = dict(pairs.HYPER)   # alpha 1e-2, beta 0.5, eta0 0.05, 'optimal', power_t 0.8
# 'optimal' at eta0 = 0.05 separates eta_P from eta_w by more than 10 % from minibatch 6 on
# ((1 + 0.025 it)^0.8 against (1 + 0.0005 it)^0.8), so the cases with moving rates go on from
# minibatch 10: a fit that has seen nine minibatches
IT0 = 10
PEGASOS = dict(alpha=0.5, beta=1.0, eta0=0.05, learning_rate="pegasos", power_t=1.0)
INVSCALING = dict(alpha=1e-2, beta=3e-2, eta0=0.2, learning_rate="invscaling", power_t=0.5)
CONSTANT = dict(fr.HP, learning_rate="constant", power_t=1.0)


def _q(v):
    return np.round(v * 64) / 64


@functools.lru_cache(maxsize=None)
def orc():
    from oracle import oracle as o

    o.build()
    o.lib()
    return o


def lane_width(k):
    return WIDTHS[0] if k <= WIDTHS[0] else WIDTHS[1] if k <= WIDTHS[1] else WIDTHS[2]


def etas(hp, first, count):
    """(eta_P, eta_w) of the minibatches first .. first + count - 1"""
    from sparsepoly_amd.pairwise import _psgd_eta

    return np.array([_psgd_eta(hp["learning_rate"], hp["eta0"], hp["alpha"], hp["beta"],
                               hp["power_t"], it) for it in range(first, first + count)])


def scores(P, w, lams, X, degree):
    """f(x) of every row of X at P (n_orders, k, d), w"""
    from sparsepoly_amd.pairwise import _rows_output

    V = np.asarray(sp.csr_matrix(X).todense(), dtype=np.double)
    return _rows_output(np.asarray(P, dtype=np.double), np.asarray(lams, dtype=np.double), V,
                        degree)[0] + V @ w


def mean_gradient(P, w, X, y, rows, lams, degree, reg, loss="squared", fit_linear=True):
    """(loss sum, gP (n_orders, d, k), gw) of the minibatch ``rows`` at P (n_orders, d, k): the
    oracle's epoch over that minibatch alone with rate 1 and no penalties"""
    o = orc()
    Pc, wc = P.copy(), w.copy()
    sl, _ = o.psgd_epoch(Pc, wc, o.CSR(X[rows]), y[rows], lams, degree, 0.0, 0.0, 0.0, reg, loss,
                         np.arange(rows.size, dtype=np.int32), fit_linear, 1.0, "constant", 1.0,
                         rows.size, 1)
    return sl, P - Pc, w - wc


# ------------------------------------------------------------------ B: the three update rules
PLAIN_HP = dict(OPTIMAL)                                  # tests/test_hip_psgd.py
PLAIN_GAMMA = {"l1": 0.003, "l21": 0.5, "squaredl12": 1e-3, "squaredl21": 2e-2}
ADA_HP = dict(alpha=1e-2, beta=1e-2, eta0=0.05)           # tests/test_hip_psgd_adagrad.py
ADA_G0, ADA_GAMMA = 1.0, {"l1": 0.2, "l21": 1.5}
FTRL_GAMMA = fr.GAMMA                                     # tests/test_hip_psgd_ftrl.py


def run_rule(rule, reg, X, y, P0, w0, lams, degree, orders, batch):
    """dict(arrays, it, loss): the device's arrays -- (P, w) and the rule's state -- after the
    epochs ``orders``, the next minibatch number and the loss sum of each epoch"""
    o = orc()
    sls = []
    if rule == "plain":
        Po, wo, it = np.ascontiguousarray(P0.swapaxes(1, 2)), w0.copy(), 1
        Xr = o.CSR(X)
        for idx in orders:
            sl, it = o.psgd_epoch(Po, wo, Xr, y, lams, degree, PLAIN_HP["alpha"],
                                  PLAIN_HP["beta"], PLAIN_GAMMA[reg], reg, "squared", idx, True,
                                  PLAIN_HP["eta0"], PLAIN_HP["learning_rate"],
                                  PLAIN_HP["power_t"], batch, it)
            sls.append(sl)
        return dict(arrays=(Po.swapaxes(1, 2).copy(), wo), it=it, loss=sls)
    if rule == "adagrad":
        P, w, it = np.ascontiguousarray(P0.swapaxes(1, 2)), w0.copy(), 1
        A_P, A_w = np.zeros(P.shape[:2]), np.zeros(w.size)
        for idx in orders:
            tot = 0.0
            for pos in range(0, idx.size, batch):
                sl, gP, gw = mean_gradient(P, w, X, y, idx[pos:pos + batch], lams, degree, reg)
                P, w = adagrad_rule(P, w, gP, gw, A_P, A_w, ADA_HP["eta0"], ADA_G0,
                                    ADA_HP["alpha"], ADA_HP["beta"], ADA_GAMMA[reg], reg)
                tot += sl
                it += 1
            sls.append(tot)
        return dict(arrays=(P.swapaxes(1, 2).copy(), w, A_P, A_w), it=it, loss=sls)
    ref = fr.Reference(o, X, y, P0, w0, lams, degree, reg, FTRL_GAMMA[reg])
    for idx in orders:
        sls.append(ref.epoch(idx, batch, FTRL_GAMMA[reg], **fr.HP))
    return dict(arrays=tuple(np.array(a) for a in ref.state()), it=ref.it, loss=sls)


# chunks: 60 x 40, degree 2, one order, two epochs, batch 7; every rule meets 129, 193 and 256,
# every regularizer 193 or 256
CHUNK_CASES = [
    ("plain", "l1", 256), ("plain", "l21", 129), ("plain", "squaredl12", 193),
    ("plain", "squaredl21", 256), ("plain", "squaredl12", 128),
    ("adagrad", "l1", 129), ("adagrad", "l21", 193), ("adagrad", "l1", 256),
    ("adagrad", "l21", 192),
    ("ftrl", "l1", 193), ("ftrl", "l21", 256), ("ftrl", "l1", 129), ("ftrl", "l21", 128),
]
CHUNK_BATCH = 7


@functools.lru_cache(maxsize=None)
def chunk_problem():
    X, y = fr._problem()
    rng = np.random.RandomState(12)
    return X, y, tuple(rng.permutation(fr.N).astype(np.int32) for _ in range(2))


def chunk_start(k):
    rng = np.random.RandomState(300 + k)
    return 0.05 * rng.randn(1, k, fr.D), 0.01 * rng.randn(fr.D), np.sign(rng.randn(k))


@functools.lru_cache(maxsize=None)
def chunk_reference(rule, reg, k):
    X, y, orders = chunk_problem()
    P0, w0, lams = chunk_start(k)
    return run_rule(rule, reg, X, y, P0, w0, lams, 2, orders, CHUNK_BATCH)


@functools.lru_cache(maxsize=None)
def chunk_pair_reference(k=193):
    """the pair epoch of tests/test_hip_psgd_dispatch.py at the fourth chunk, batch 7"""
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z, S, y, t, I, order = pairs.problem()
    P0, w0, lams = pairs.params(k)
    return restate_pairwise_epoch(P0, w0, lams, X, Z, t, pairs.DEGREE, "logistic", "l1",
                                  gamma=pairs.GAMMA, batch_size=7, fit_linear=True, it=1,
                                  **pairs.HYPER)


# strides: one epoch of two minibatches of 30 rows
STRIDE_SHAPES = tuple((k, K_NB * (K_BLOCK // lane_width(k)) + 37) for k in (8, 24, 40)) \
    + ((4, K_NB * K_BLOCK + 37),)
STRIDE_CASES = [(rule, reg, k, d) for (k, d) in STRIDE_SHAPES
                for rule in ("plain", "adagrad", "ftrl") for reg in ("l1", "l21")] \
    + [("plain", "squaredl12", 40, STRIDE_SHAPES[2][1])]
STRIDE_ROWS, STRIDE_BATCH = 60, 30


def stride_trips(k, d):
    """(columns per trip of the column loop, of the w loop)"""
    return K_NB * (K_BLOCK // lane_width(k)), K_NB * K_BLOCK


@functools.lru_cache(maxsize=None)
def stride_problem(k, d):
    """X (60, d) storing a dozen columns -- in the first trip of the column loop, in the second,
    the first column of the second trip, column d - 1, and for d beyond the w loop's first trip
    the same around that boundary -- and nothing else; y, the start, one visiting order"""
    T, TW = stride_trips(k, d)
    stored = {0, 1, 5, 100, T - 1, T, T + 1, T + 20, d - 1, d - 2}
    if d > TW:
        stored |= {2 * T + 3, 5 * T, TW - 1, TW, TW + 3}
    stored = np.array(sorted(stored))
    assert stored.max() == d - 1
    rng = np.random.RandomState(7 * k + 1)
    A = sp.lil_matrix((STRIDE_ROWS, d))
    for i in range(STRIDE_ROWS):
        n = rng.randint(4, 7)
        cols = set(rng.choice(stored, size=n, replace=False)) | {stored[i % stored.size]}
        for c in sorted(cols):
            A[i, c] = _q(rng.uniform(0.25, 1.0)) * np.sign(rng.randn())
    X = sp.csr_matrix(A)
    y = _q(rng.randn(STRIDE_ROWS))
    P0, w0, lams = 0.3 * rng.randn(1, k, d), 0.01 * rng.randn(d), np.sign(rng.randn(k))
    return X, y, P0, w0, lams, (rng.permutation(STRIDE_ROWS).astype(np.int32),), stored


@functools.lru_cache(maxsize=None)
def stride_reference(rule, reg, k, d):
    X, y, P0, w0, lams, orders, _ = stride_problem(k, d)
    return run_rule(rule, reg, X, y, P0, w0, lams, 2, orders, STRIDE_BATCH)


def rule_start_state(rule, reg, P0, w0):
    """the arrays of ``run_rule`` before the first minibatch"""
    from sparsepoly_amd.pairwise import ftrl_start

    if rule == "plain":
        return P0, w0
    if rule == "adagrad":
        return P0, w0, np.zeros((P0.shape[0], P0.shape[2])), np.zeros(w0.size)
    return (P0, w0) + ftrl_start(P0, w0, G0, fr.HP["eta0"], fr.HP["alpha"], fr.HP["beta"],
                                 FTRL_GAMMA[reg], reg)


# ------------------------------------------------------------------ A: FTRL, pointwise routes
def _signs(P0, w0, lams, X, degree):
    f = scores(P0, w0, lams, X, degree)
    return np.where(f >= 0, 1.0, -1.0)


def _revival_start(k, n_orders):
    """fr._start with three live columns made tiny: near the threshold, they can die"""
    P0, w0, lams = fr._start(k, n_orders)
    P0[:, :, list(TINY)] *= 2e-4
    return P0, w0, lams


# Column ZERO of fr._problem (P0 = 0) gathers |z| ~ 0.8 in two epochs: gamma below that revives it.
# A live column dies when a gradient carries its z inside the threshold; for l21 that needs a
# column whose z starts just outside (a tiny p) and whose gradients are small against gamma
# (entries scaled by 1/16, still exact in f32).
TINY = (2, 17, 31)
REVIVE_GAMMA = {"l1": 0.1, "l21": 0.5}
POINT_CASES = {
    # name: reg, k, degree, n_orders, batch, schedule, first minibatch, loss, fit_linear, det
    "optimal-l1": dict(reg="l1", k=8, degree=2, n_orders=1, batch=7, hp=OPTIMAL, it0=IT0),
    "optimal-l21": dict(reg="l21", k=33, degree=3, n_orders=2, batch=7, hp=OPTIMAL, it0=IT0),
    "invscaling": dict(reg="l1", k=70, degree=2, n_orders=1, batch=7, hp=INVSCALING, it0=1),
    "pegasos": dict(reg="l21", k=16, degree=2, n_orders=1, batch=7, hp=PEGASOS, it0=IT0),
    "det-l1": dict(reg="l1", k=70, degree=3, n_orders=2, batch=7, hp=OPTIMAL, it0=IT0, det=1),
    "det-l21": dict(reg="l21", k=8, degree=2, n_orders=1, batch=7, hp=OPTIMAL, it0=IT0, det=1),
    "logistic": dict(reg="l1", k=33, degree=2, n_orders=1, batch=7, hp=OPTIMAL, it0=IT0,
                     loss="logistic"),
    "hinge": dict(reg="l1", k=8, degree=2, n_orders=1, batch=1, hp=CONSTANT, it0=1,
                  loss="squared_hinge"),
    "nolinear": dict(reg="l21", k=8, degree=3, n_orders=2, batch=7, hp=OPTIMAL, it0=IT0,
                     fit_linear=False),
    "revive-l1": dict(reg="l1", k=30, degree=2, n_orders=1, batch=7, hp=CONSTANT, it0=1,
                      gamma=REVIVE_GAMMA["l1"], start="revival"),
    "revive-l21": dict(reg="l21", k=30, degree=2, n_orders=1, batch=7, hp=CONSTANT, it0=1,
                       gamma=REVIVE_GAMMA["l21"], start="revival"),
}


def point_case(name):
    """the case with its defaults filled in, its problem, start and visiting orders"""
    c = dict(dict(loss="squared", fit_linear=True, det=0, start="plain"), **POINT_CASES[name])
    c.setdefault("gamma", FTRL_GAMMA[c["reg"]])
    X, y = fr._problem()
    start = fr._start
    if c["start"] == "revival":
        start = _revival_start
        X = sp.csr_matrix(X.multiply(np.where(np.isin(np.arange(fr.D), TINY), 1 / 16.0, 1.0)))
    P0, w0, lams = start(c["k"], c["n_orders"])
    if c["loss"] != "squared":
        y = _signs(P0, w0, lams, X, c["degree"])
    rng = np.random.RandomState(2)
    orders = [rng.permutation(fr.N).astype(np.int32) for _ in range(2)]
    return c, X, y, P0, w0, lams, orders


@functools.lru_cache(maxsize=None)
def point_reference(name):
    """dict(arrays (P, w, z_P, z_w, n_P, n_w), it, loss [per epoch]); for 'hinge' also ``past``:
    per epoch the positions of the order whose row lay past the margin when it was visited,
    ``clear``: the smallest |y f - 1| over all visits of stored rows, and ``lazy``: the number of
    those visits that met a column with n_P > 0"""
    c, X, y, P0, w0, lams, orders = point_case(name)
    hp = c["hp"]
    ref = fr.Reference(orc(), X, y, P0, w0, lams, c["degree"], c["reg"], c["gamma"], c["loss"],
                       c["fit_linear"], hp, c["it0"])
    out = dict(loss=[], past=[], clear=np.inf, lazy=0)
    for idx in orders:
        if name != "hinge":
            out["loss"].append(ref.epoch(idx, c["batch"], c["gamma"], **hp))
            continue
        tot, past = 0.0, []
        for pos in range(idx.size):
            row = int(idx[pos])
            before = [np.array(a) for a in ref.state()]
            if X[row].nnz:
                m = y[row] * scores(before[0], before[1], lams, X[row], c["degree"])[0]
                out["clear"] = min(out["clear"], abs(m - 1.0))
                if m > 1.0:
                    past.append(pos)
                    out["lazy"] += int((before[4][0, X[row].indices] > 0).any())
            tot += ref.epoch(idx[pos:pos + 1], 1, c["gamma"], **hp)
            if X[row].nnz and m > 1.0:   # g = 0: the rule leaves every bit
                assert all(np.array_equal(a, b) for a, b in zip(before, ref.state()))
        out["loss"].append(tot)
        out["past"].append(np.array(past, dtype=np.int64))
    out.update(arrays=tuple(np.array(a) for a in ref.state()), it=ref.it)
    return out


# ------------------------------------------------------------------ A: FTRL, pair and list routes
PAIR_GAMMA = {"l1": 0.5, "l21": 2.0}   # against |z| ~ |p| (G0 / eta0 + beta) ~ 0.25 * 16.5
PAIR_KS = (16, 33, 70)
PAIR_ROUTES = ("pairs", "weighted", "sampled", "det")
PAIR_CASES = [(route, reg, PAIR_KS[(2 * i + j + b) % 3], batch)
              for i, route in enumerate(PAIR_ROUTES) for j, reg in enumerate(("l1", "l21"))
              for b, batch in enumerate((1, 7))]
SAMPLE = dict(pairs.SAMPLE)            # one negative, the hardest of 4
N_LIST, M_LIST, LIST_BATCH = 12, 3, 5  # 12 lists: minibatches of 5, 5 and a ragged 2


@functools.lru_cache(maxsize=None)
def pair_weights():
    """one weight per triple, zeros among them (exact in f32)"""
    rng = np.random.RandomState(21)
    return rng.choice([0.0, 0.0, 0.5, 1.0, 1.5, 2.0], size=pairs.N_TRIPLES)


@functools.lru_cache(maxsize=None)
def list_triples():
    """12 lists of one positive and three distinct negatives, grouped"""
    rng = np.random.RandomState(22)
    rows = []
    for q in range(N_LIST):
        c = rng.choice(pairs.N_CAND, size=M_LIST + 1, replace=False)
        rows += [(q % pairs.N_CTX, c[0], c[i]) for i in range(1, M_LIST + 1)]
    return np.array(rows, dtype=np.int32)


def pair_epoch_ref(P, w, state, it, triples, reg, batch, hp=OPTIMAL, fit_linear=True,
                   weights=None, wide=False, gamma=None, k=None):
    """one epoch of ``restate_pairwise_epoch`` under FTRL -> (P, w, sum_loss, it, state)"""
    from sparsepoly_amd.pairwise import restate_pairwise_epoch

    X, Z = pairs.problem()[:2]
    lams = pairs.params(P.shape[1])[2]
    return restate_pairwise_epoch(P, w, lams, X, Z, triples, pairs.DEGREE, "logistic", reg,
                                  gamma=PAIR_GAMMA[reg] if gamma is None else gamma,
                                  batch_size=batch, fit_linear=fit_linear, it=it, wide=wide,
                                  weights=weights, ftrl=G0, state=state, **hp)


@functools.lru_cache(maxsize=None)
def pair_reference(route, reg, k, batch, hp_name="optimal", fit_linear=True, wide=False,
                   zero_weights=False):
    """two epochs of a pair route under FTRL, the state carried: dict(arrays, it, loss, triples
    [per epoch, context / candidate numbering])"""
    from sparsepoly_amd.pairwise import restate_sample

    X, Z, S, y, t, I, order = pairs.problem()
    hp = {"optimal": OPTIMAL, "pegasos": PEGASOS, "invscaling": INVSCALING}[hp_name]
    P, w, lams = pairs.params(k)
    wt = None
    if route == "weighted":
        wt = np.zeros(pairs.N_TRIPLES) if zero_weights else pair_weights()
    it, state, sls, used = IT0, None, [], []
    for ep in range(2):
        tt = t
        if route == "sampled":
            tt = restate_sample(P, w, lams, X, Z, I, pairs.DEGREE, SAMPLE["n_neg"], SAMPLE["M"],
                                SAMPLE["max_draws"], SAMPLE["seed"], ep)[0]
        P, w, sl, it, state = pair_epoch_ref(P, w, state, it, tt, reg, batch, hp, fit_linear, wt,
                                             wide)
        sls.append(float(sl))
        used.append(tt)
    return dict(arrays=(P, w) + tuple(state), it=it, loss=sls, triples=used)


@functools.lru_cache(maxsize=None)
def list_reference(reg, k, wide=False):
    from sparsepoly_amd.pairwise import restate_list_epoch

    X, Z = pairs.problem()[:2]
    P, w, lams = pairs.params(k)
    it, state, sls = IT0, None, []
    for ep in range(2):
        P, w, sl, it, state = restate_list_epoch(
            P, w, lams, X, Z, list_triples(), M_LIST, pairs.DEGREE, "list", "logistic", reg,
            gamma=PAIR_GAMMA[reg], batch_size=LIST_BATCH, fit_linear=True, it=it, wide=wide,
            ftrl=G0, state=state, **OPTIMAL)
        sls.append(float(sl))
    return dict(arrays=(P, w) + tuple(state), it=it, loss=sls)


def pair_start_state(reg, k, hp=OPTIMAL):
    from sparsepoly_amd.pairwise import ftrl_start

    P0, w0, _ = pairs.params(k)
    return (P0, w0) + ftrl_start(P0, w0, G0, hp["eta0"], hp["alpha"], hp["beta"], PAIR_GAMMA[reg],
                                 reg)


@functools.lru_cache(maxsize=None)
def round_trip_state(k=70, n_orders=2):
    """a state no epoch produced: every entry of z_P distinct, n >= 0"""
    rng = np.random.RandomState(23)
    return (rng.randn(n_orders, k, fr.D), rng.randn(fr.D), rng.rand(n_orders, fr.D) ** 2,
            rng.rand(fr.D) ** 2)


# ================================================================== the host tests
def test_device_constants():
    """the stride and chunk shapes of this module and of tests/test_hip_psgd_update_shapes.py are
    derived from these four: they must move with them"""
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def const(header, name):
        m = re.search(r"constexpr int %s = (\d+);" % name, text(header))
        assert m, name
        return int(m.group(1))

    m = re.search(r"#define SPFM_DISPATCH_L\(.*?\n\n", text("spfm_engine.hip.h"), flags=re.S)
    got = (const("spfm_common.hip.h", "kBlock"), const("spfm_psgd.hip.h", "kPsgdNB"),
           const("spfm_psgd.hip.h", "kPsgdMaxC"),
           tuple(int(v) for v in re.findall(r"constexpr int L = (\d+);", m.group(0))))
    assert got == (256, 1024, 4, (16, 32, 64)) == (K_BLOCK, K_NB, K_MAXC, WIDTHS), (
        "kBlock, kPsgdNB, kPsgdMaxC or the widths of SPFM_DISPATCH_L changed (%r): the shapes of "
        "tests/test_psgd_update_shapes_host.py (STRIDE_SHAPES, CHUNK_CASES) must move with them"
        % (got,))
    assert STRIDE_SHAPES == ((8, 16384 + 37), (24, 8192 + 37), (40, 4096 + 37),
                             (4, 262144 + 37))
    ks = {k for _, _, k in CHUNK_CASES}
    assert ks == {128, 129, 192, 193, 256} and max(ks) == 64 * K_MAXC
    for rule in ("plain", "adagrad", "ftrl"):
        assert {129, 193, 256} <= {k for r, _, k in CHUNK_CASES if r == rule}
    for reg in PLAIN_GAMMA:
        assert {k for _, r, k in CHUNK_CASES if r == reg} & {193, 256}


def _moved(ref, start, least=1e-4):
    assert all(np.isfinite(a).all() for a in ref["arrays"])
    assert np.abs(ref["arrays"][0] - start[0]).max() > least
    assert np.abs(ref["arrays"][1] - start[1]).max() > least


@pytest.mark.parametrize("rule,reg,k", CHUNK_CASES)
def test_chunk_references(rule, reg, k):
    ref = chunk_reference(rule, reg, k)
    P0, w0, _ = chunk_start(k)
    _moved(ref, (P0, w0))
    assert ref["it"] == 1 + 2 * -(-fr.N // CHUNK_BATCH)
    P = ref["arrays"][0]
    for c in range(-(-k // 64)):   # every chunk of the components moved
        assert np.abs(P[:, 64 * c:64 * (c + 1)] - P0[:, 64 * c:64 * (c + 1)]).max() > 1e-4
    if rule == "ftrl":
        for a, b in zip(ref["arrays"], rule_start_state(rule, reg, P0, w0)):
            assert np.array_equal(a[..., fr.NEVER], b[..., fr.NEVER])


def test_chunk_pair_reference():
    Pr, wr, sl, it = chunk_pair_reference()
    P0, w0, _ = pairs.params(193)
    assert it == 1 + 6 and np.abs(Pr[:, 192] - P0[:, 192]).max() > 1e-4
    assert np.abs(wr - w0).max() > 1e-4


@pytest.mark.parametrize("rule,reg,k,d", STRIDE_CASES)
def test_stride_references(rule, reg, k, d):
    X, y, P0, w0, lams, orders, stored = stride_problem(k, d)
    T, TW = stride_trips(k, d)
    assert T < d < 2 * T or d > TW   # the column loop, and for the last shape the w loop, wraps
    assert np.array_equal(np.unique(X.indices), stored)
    assert {T, d - 1} <= set(stored) and (stored < T).sum() >= 4 and (stored >= T).sum() >= 4
    ref = stride_reference(rule, reg, k, d)
    start = rule_start_state(rule, reg, P0, w0)
    _moved(ref, start)
    assert ref["it"] == 3
    never = np.setdiff1d(np.arange(d), stored)
    assert (never < T).sum() > 3 and (never >= T).sum() > 3
    second = stored[stored >= T]
    if d > TW:
        assert {TW - 1, TW, TW + 3} <= set(stored)
        second = np.concatenate([second, stored[stored >= TW]])
    # the second-trip columns received a non-zero gradient, in P and in w
    assert (np.abs(ref["arrays"][0] - P0)[0][:, second].max(axis=0) > 1e-6).all()
    assert (np.abs(ref["arrays"][1] - w0)[second] > 1e-9).all()
    if rule == "ftrl":     # lazy: the never-stored columns keep every bit, in both trips
        assert (ref["arrays"][4][0, stored] > 0).all() and (ref["arrays"][5][stored] > 0).all()
        for a, b in zip(ref["arrays"], start):
            assert np.array_equal(a[..., never], b[..., never])
    else:                  # they shrink: every column changes
        assert (ref["arrays"][1][never] != w0[never]).all()
        if reg in ("l1", "l21"):
            assert ((ref["arrays"][0] != P0)[0].any(axis=0))[never].all()


@pytest.mark.parametrize("name", sorted(POINT_CASES))
def test_point_references(name):
    c, X, y, P0, w0, lams, orders = point_case(name)
    ref = point_reference(name)
    P, w, zP, zw, nP, nw = ref["arrays"]
    assert all(np.isfinite(a).all() for a in ref["arrays"]) and np.abs(P).max() < 10
    assert np.abs(P - P0).max() > 1e-4
    nbat = 2 * -(-fr.N // c["batch"])
    assert ref["it"] == c["it0"] + nbat
    e = etas(c["hp"], c["it0"], nbat)
    if c["hp"]["learning_rate"] in ("optimal", "pegasos"):
        assert (np.abs(e[:, 0] - e[:, 1]) > 0.1 * e.max(axis=1)).all(), e
    if c["hp"]["learning_rate"] != "constant":   # ... and both move with every minibatch
        assert (np.diff(e, axis=0) < 0).all()
    if c["fit_linear"]:
        assert np.abs(w - w0).max() > 1e-4
    else:
        from sparsepoly_amd.pairwise import ftrl_start
        s = ftrl_start(P0, w0, G0, c["hp"]["eta0"], c["hp"]["alpha"], c["hp"]["beta"], c["gamma"],
                       c["reg"])
        assert np.array_equal(w, w0) and np.array_equal(zw, s[1]) and not nw.any()
    if name == "hinge":
        past = ref["past"]
        assert min(p.size for p in past) >= 3 and max(p.size for p in past) <= fr.N - 10
        assert ref["clear"] > 1e-6 and ref["lazy"] >= 3
    if c["start"] == "revival":
        if c["reg"] == "l1":     # per component
            assert (P[P0 == 0] != 0).any() and (P[P0 != 0] == 0).any()
        else:                    # per column
            live0, live = np.abs(P0).max(axis=1) > 0, np.abs(P).max(axis=1) > 0
            assert (live & ~live0).any() and (live0 & ~live).any()
            assert (nP[live0 & ~live] > 0).all()   # (dead by the threshold, not never touched)


@pytest.mark.parametrize("route,reg,k,batch", PAIR_CASES)
def test_pair_references(route, reg, k, batch):
    ref = pair_reference(route, reg, k, batch)
    start = pair_start_state(reg, k)
    _moved(ref, start)
    nbat = 2 * -(-ref["triples"][0].shape[0] // batch)
    assert ref["it"] == IT0 + nbat
    e = etas(OPTIMAL, IT0, nbat)
    assert (np.abs(e[:, 0] - e[:, 1]) > 0.1 * e.max(axis=1)).all()
    assert (np.diff(e, axis=0) < 0).all()
    if route == "weighted":
        wt = pair_weights()
        assert (wt == 0).any() and (wt > 0).any()
        if batch > 1:
            mixed = [(wt[p:p + batch] == 0).any() and (wt[p:p + batch] > 0).any()
                     for p in range(0, wt.size, batch)]
            assert any(mixed) and wt.size % batch == 5     # ... and a ragged last minibatch
    if route == "sampled":
        assert ref["triples"][0].shape == (pairs.problem()[5].nnz, 3)
        assert not np.array_equal(ref["triples"][0], ref["triples"][1])


def test_pair_schedules_and_edges():
    for hp_name, hp in (("pegasos", PEGASOS), ("invscaling", INVSCALING)):
        ref = pair_reference("pairs", "l1", 33, 7, hp_name)
        _moved(ref, pair_start_state("l1", 33, hp))
        e = etas(hp, IT0, 12)
        assert (np.diff(e, axis=0) < 0).all()
        if hp_name == "pegasos":
            assert (np.abs(e[:, 0] - e[:, 1]) > 0.1 * e.max(axis=1)).all()
    ref = pair_reference("pairs", "l21", 16, 7, "optimal", False)   # fit_linear off
    start = pair_start_state("l21", 16)
    assert np.abs(ref["arrays"][0] - start[0]).max() > 1e-4
    for i in (1, 3, 5):
        assert np.array_equal(ref["arrays"][i], start[i])
    ref = pair_reference("weighted", "l1", 70, 7, "optimal", True, False, True)   # all weights 0
    assert ref["it"] == IT0 + 12 and ref["loss"] == [0.0, 0.0]
    for a, b in zip(ref["arrays"], pair_start_state("l1", 70)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("reg,k", [("l1", 33), ("l21", 70)])
def test_list_references(reg, k):
    t = list_triples()
    from sparsepoly_amd.pairwise import check_lists
    check_lists(t, M_LIST, "list")
    assert (t[:, 1] != t[:, 2]).all()
    ref = list_reference(reg, k)
    _moved(ref, pair_start_state(reg, k))
    assert ref["it"] == IT0 + 2 * 3
