"""``spfm_bank_group_sums`` and ``ModelBank.group_sums`` on the device.  Needs a real MI355X:
``pytest -m gpu``.

The tables are compared with ``restate_group_sums(restate_bank_scores(..., wide=True), ...,
wide=True)``.  The bound comes from the order documented at ``bank_group_partial_kernel``
(``csrc/spfm_bank.hip.h``) and from no device run.  Per cell (metric q, member f, group g)

    sum_{i in g} w_i * terms_i  +  (N_sum + 3) 2^-53 sum_{i in g} w_i * metric_i

``terms_i`` is how far the metric of a score within the score's bound of the exact one can be from
the exact metric, plus the roundings of the metric's own evaluation: ``_loss_terms`` of
``tests/test_hip_bank.py`` for the three losses; ``b + 2^-53 (|p| + |y| + b)`` for ``abs_error``
(slope 1, one subtraction); for ``sign_error`` 0 where the score cannot change sides (``|p| > b``,
or ``b = 0``: an empty row's score is exact on both sides) and 1 elsewhere.

``N_sum`` is the largest number of additions a row's term goes through.  From the kernel comment:
the wave that owns the row adds the terms of its 64 rows one after the other (at most 64), the four
waves of the block are added in wave order (4), the finish adds the call's P blocks of 256 rows in
block order (P): ``N_sum = 64 + 4 + P``.  One slab of n rows has ``P = ceil(n / 256)`` blocks;
every slab starts a new block, so with many slabs ``P <= n`` (at most one block per row).  The 3
covers the rounding of the product ``w_i * value``, the second-order terms and the ``longdouble``
reference.

``sign_error`` with integer weights is a sum of small integers: exact in any order, so the device
table equals NumPy's bit for bit once no score can change sides; the NumPy side asserts that
(every restated ``|score|`` above its own bound by a factor of 1 + 1e-9, no row left out) before
the device is touched.  Each case prints its largest error as a fraction of its bound.
"""
import ctypes as C

import numpy as np
import pytest
from test_explain_host import rows_matrix
from test_hip_bank import CLEAR, U, _check, _loss_case, _loss_terms, _reference
from test_ranking_host import fm

pytestmark = pytest.mark.gpu

NAMES = ("squared", "squared_hinge", "logistic", "abs_error", "sign_error")
N = 600
G5 = 5  # groups 0..2 hold rows, 3 holds none, the rows of 4 all weigh 0


def _terms(metric, p, y, b):
    if metric == "abs_error":
        return b + U * (np.abs(p) + np.abs(y) + b)
    if metric == "sign_error":
        return np.where((np.abs(p) > b) | (b == 0), 0.0, 1.0).astype(np.longdouble)
    return _loss_terms(metric, p, y, b)


def _by_group(M, w, g, G):
    """(F, G): sum over the rows of each group of w_i M[i, f], in longdouble"""
    out = np.zeros((M.shape[1], G), dtype=np.longdouble)
    wl = np.ones(M.shape[0], dtype=np.longdouble) if w is None else w.astype(np.longdouble)
    g = np.zeros(M.shape[0], dtype=int) if g is None else g
    for k in range(G):
        out[:, k] = (wl[:, None] * M)[g == k].sum(axis=0)
    return out


def _check_tables(got, ref, y, w, g, G, metrics, P, what):
    """every table of ``got`` against the restatement, within the documented bound"""
    from sparsepoly_amd.bank import _metric, restate_group_sums

    want, bound, _ = ref
    t2 = y[:, None] if y.ndim == 1 else y
    exact = restate_group_sums(want, y, w, g, G, metrics, wide=True)
    n_sum = 64 + 4 + P
    for q, m in enumerate(metrics):
        if m == "logistic":  # no score within reach of the branch points
            assert (np.abs(np.abs(want * t2) - 18) > 1e-6).all()
        vals = _metric(m, want, t2, np.longdouble)
        tol = _by_group(_terms(m, want, t2, bound), w, g, G) + (n_sum + 3) * U * _by_group(
            vals, w, g, G)
        assert got[m].shape == (want.shape[1], G) and got[m].dtype == np.float64
        _check(got[m], exact[q], tol, "%s, %s" % (what, m))
    wsum = np.bincount(np.zeros(len(y), dtype=int) if g is None else g, weights=w, minlength=G)
    assert (got["weight"] == wsum).all()


def _grouping(n, seed=21):
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 3, size=n).astype(np.int32)
    g[rng.rand(n) < 0.1] = 4
    w = rng.rand(n) * 2
    w[g == 4] = 0.0
    w[rng.rand(n) < 0.05] = 0.0  # zero weights inside the other groups too
    return g, w


@pytest.fixture(scope="module")
def case():
    """the members (k = 3, 30, 65), rows and targets of test_hip_bank's loss case, its reference
    computed once, and a grouping of the 600 rows"""
    ests, X, y, Y, ref = _loss_case()
    assert X.shape[0] == N and (np.diff(X.indptr) == 0).any()
    g, w = _grouping(N)
    assert not (g == 3).any() and (g == 4).any() and (w[g == 4] == 0).all()
    return ests, X, y, Y, ref, g, w


@pytest.fixture(scope="module")
def bank(case):
    from sparsepoly_amd import ModelBank

    with ModelBank(case[0]) as b:
        yield b


# ---------------------------------------------------------------- 1. values
@pytest.mark.parametrize("metric", NAMES)
def test_values(case, bank, metric):
    """600 rows = 3 blocks of 256, one slab: P = 3"""
    ests, X, y, Y, ref, g, w = case
    for t, what in ((y, "shared y"), (Y, "per-member Y")):
        got = bank.group_sums(X, t, groups=g, n_groups=G5, sample_weight=w, metrics=(metric,))
        assert set(got) == {metric, "weight"}
        _check_tables(got, ref, t, w, g, G5, (metric,), 3, what)
        assert (got[metric][:, 3] == 0).all() and (got[metric][:, 4] == 0).all()


def test_four_metrics_in_one_pass_equal_their_own_passes(case, bank):
    ests, X, y, Y, ref, g, w = case
    four = ("logistic", "abs_error", "sign_error", "squared")
    got = bank.group_sums(X, Y, groups=g, n_groups=G5, sample_weight=w, metrics=four)
    _check_tables(got, ref, Y, w, g, G5, four, 3, "Q = 4")
    for m in four:  # a metric's sums do not depend on the metrics beside it
        alone = bank.group_sums(X, Y, groups=g, n_groups=G5, sample_weight=w, metrics=(m,))
        assert (alone[m] == got[m]).all()


@pytest.mark.parametrize("G", [1, 3, 32])
def test_number_of_groups(case, bank, G):
    ests, X, y, Y, ref, _, w = case
    g = (np.arange(N) * 7 % G).astype(np.int32)
    got = bank.group_sums(X, y, groups=g, n_groups=G, sample_weight=w,
                          metrics=("squared", "sign_error"))
    _check_tables(got, ref, y, w, g, G, ("squared", "sign_error"), 3, "G = %d" % G)


def test_no_groups_no_weights_and_the_default_loss(case, bank):
    ests, X, y, Y, ref, g, w = case
    got = bank.group_sums(X, y)  # regressors: 'loss' is 'squared'
    assert set(got) == {"loss", "weight"} and got["loss"].shape == (3, 1)
    assert got["weight"][0] == N
    _check_tables({"squared": got["loss"], "weight": got["weight"]}, ref, y, None, None, 1,
                  ("squared",), 3, "groups=None, sample_weight=None")
    only_g = bank.group_sums(X, y, groups=g, n_groups=G5, metrics=("abs_error",))
    _check_tables(only_g, ref, y, None, g, G5, ("abs_error",), 3, "sample_weight=None")
    only_w = bank.group_sums(X, y, sample_weight=w, metrics=("abs_error",))
    _check_tables(only_w, ref, y, w, None, 1, ("abs_error",), 3, "groups=None")


@pytest.mark.parametrize("F", [1, 5, 64])
def test_number_of_members(F):
    """333 rows: no multiple of 64 or of 256, the last wave of the second block holds 13 rows"""
    from sparsepoly_amd import ModelBank

    ests = [fm(2, 4, 40, None, True, seed=500 + f) for f in range(F)]
    for e in ests:
        e.P_ *= 0.5
        e.w_ *= 0.3
    n = 333
    X = rows_matrix(([0, 1, 5, 40, 12, 7, 3, 9] * 42)[:n], 40, seed=F)
    rng = np.random.RandomState(F)
    Y = np.where(rng.rand(n, F) < 0.5, -1.0, 1.0)
    g, w = _grouping(n, seed=F)
    ref = _reference(ests, X)
    with ModelBank(ests) as b:
        got = b.group_sums(X, Y, groups=g, n_groups=G5, sample_weight=w,
                           metrics=("squared_hinge", "abs_error"))
        if F == 64:  # both caps at once: the 64 KB table
            g32 = (np.arange(n) * 5 % 32).astype(np.int32)
            full = b.group_sums(X, Y, groups=g32, n_groups=32, sample_weight=w,
                                metrics=("logistic", "sign_error"))
    _check_tables(got, ref, Y, w, g, G5, ("squared_hinge", "abs_error"), 2, "F = %d" % F)
    if F == 64:
        _check_tables(full, ref, Y, w, g32, 32, ("logistic", "sign_error"), 2, "F = 64, G = 32")


def test_many_slabs(case, bank):
    """slabs of at most 50 stored entries: more than 10 slabs, every one starts a new block, so
    the finish adds up to one block per row: N_sum = 64 + 4 + n.  The groups are spread over every
    slab."""
    ests, X, y, Y, ref, g, w = case
    bank.set_partition(50)
    try:
        got = bank.group_sums(X, Y, groups=g, n_groups=G5, sample_weight=w, metrics=NAMES[:4])
        assert bank.info()["slabs"] > 10
        again = bank.group_sums(X, Y, groups=g, n_groups=G5, sample_weight=w, metrics=NAMES[:4])
    finally:
        bank.set_partition(0)
    _check_tables(got, ref, Y, w, g, G5, NAMES[:4], N, "slabs of 50 entries")
    for m in NAMES[:4]:
        assert (got[m] == again[m]).all()


# ---------------------------------------------------------------- 2. sign_error: exact
def test_sign_error_with_integer_weights_is_exact():
    """degree 3 'augment' with a linear term: the dummy column gives the empty rows a score too"""
    from sparsepoly_amd import ModelBank
    from sparsepoly_amd.bank import restate_group_sums

    ests = [fm(3, k, 40, "augment", True, seed=82 + k) for k in (3, 30, 65)]
    X = rows_matrix([0, 1, 5, 40, 12, 7, 3, 9] * 75, 40, seed=13)
    want, bound, _ = _reference(ests, X)
    # NumPy side first: no score can change sides, no row is left out
    assert (np.abs(want) > bound * (1 + CLEAR)).all()
    rng = np.random.RandomState(14)
    y = np.where(rng.rand(N) < 0.5, -1.0, 1.0)
    w = rng.randint(0, 4, size=N).astype(np.double)
    g = rng.randint(0, 3, size=N).astype(np.int32)
    exact = restate_group_sums(want, y, w, g, 3, ("sign_error",))[0]
    assert exact.min() > 0 and (exact < (w.sum())).all()  # both answers occur
    with ModelBank(ests) as b:
        got = b.group_sums(X, y, groups=g, sample_weight=w, metrics=("sign_error",))
        b.set_partition(50)
        parts = b.group_sums(X, y, groups=g, sample_weight=w, metrics=("sign_error",))
    assert (got["sign_error"] == exact).all() and (parts["sign_error"] == exact).all()
    assert (got["weight"] == np.bincount(g, weights=w)).all()


# ---------------------------------------------------------------- 3. contracts
def test_contracts(case):
    from sparsepoly_amd import ModelBank

    ests, X, y, Y, ref, g, w = case
    kw = dict(groups=g, n_groups=G5, metrics=("logistic", "abs_error"))
    with ModelBank(ests) as b:
        before = b.losses(X, y), b.losses(X, Y, loss="logistic", mean=True)
        one = b.group_sums(X, Y, sample_weight=w, **kw)
        two = b.group_sums(X, Y, sample_weight=w, **kw)
        unit = b.group_sums(X, Y, sample_weight=np.ones(N), **kw)
        none = b.group_sums(X, Y, **kw)
        # losses(sample_weight=): the G = 1 table; mean divides by sum(w)
        wl = b.losses(X, y, sample_weight=w)
        tab = b.group_sums(X, y, sample_weight=w)
        assert (wl == tab["loss"][:, 0]).all()
        assert tab["weight"][0] == np.bincount(np.zeros(N, dtype=int), weights=w)[0]
        assert (b.losses(X, y, sample_weight=w, mean=True) == wl / tab["weight"][0]).all()
        # the G = 1 unweighted table against bank.losses: the same bound, other orders
        flat = b.group_sums(X, y)["loss"][:, 0]
        # without weights losses() takes its own path: the bits of before any group_sums call
        after = b.losses(X, y), b.losses(X, Y, loss="logistic", mean=True)
    for m in kw["metrics"]:
        assert (one[m] == two[m]).all()        # run to run
        assert (unit[m] == none[m]).all()      # a weight of 1.0 changes no bit
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    want, bound, _ = ref
    from sparsepoly_amd.bank import _metric

    vals = _metric("squared", want, y[:, None], np.longdouble)
    slack = _loss_terms("squared", want, y[:, None], bound).sum(axis=0)
    tol = 2 * slack + ((64 + 4 + 3 + 3) + (20 + 1 + 2)) * U * vals.sum(axis=0)
    _check(flat, before[0].astype(np.longdouble), tol, "G = 1 table against bank.losses")
    # column f of the mixed bank is the one-member bank of member f, bit for bit
    for f, e in enumerate(ests):
        with ModelBank([e]) as solo:
            col = solo.group_sums(X, Y[:, f], sample_weight=w, **kw)
        for m in kw["metrics"]:
            assert col[m].shape == (1, G5) and (col[m][0] == one[m][f]).all()


# ---------------------------------------------------------------- 4. the C entry point's errors
def test_entry_point_refusals():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    lib = eng._lib
    d, F, k, n = 6, 2, 3, 3
    X = rows_matrix([2, 0, 3], d, seed=1)
    ip, ii, dd = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    i32, i64, f64 = C.c_int32, C.c_int64, C.c_double
    y = np.ones(n)
    sq = np.array([_capi.BANK_METRICS["squared"]], dtype=np.int32)
    out = np.full(8 * F * 40, 7.25)

    def call(n_=n, y_=y, w=None, g=None, G=2, Q=1, m=sq, o=out):
        return lib.spfm_bank_group_sums(eng._h, n_, d, p(ip, i64), p(ii, i32), p(dd, f64),
                                        p(y_, f64), 0, p(w, f64), p(g, i32), G, Q, p(m, i32),
                                        p(o, f64))

    def expect(rc, code, text):
        msg = lib.spfm_last_error(eng._h).decode()
        assert rc == code and text in msg, (rc, msg)
        assert (out == 7.25).all()  # refused before the first write

    INV, UNS = _capi.SPFM_ERR_INVALID, _capi.SPFM_ERR_UNSUPPORTED
    ids = lambda *a: np.array(a, dtype=np.int32)  # noqa: E731
    try:
        expect(call(), INV, "no bank set")
        eng.bank_set(np.array([0, k, 2 * k]), [2], np.zeros((1, d, 2 * k)), np.ones(2 * k),
                     np.zeros((d, F)))
        expect(call(g=ids(0, 2, 1)), INV, "group id 2 of row 1")
        expect(call(g=ids(0, -1, 1)), INV, "group id -1")
        expect(call(w=np.array([1.0, -0.5, 1.0])), INV, "negative or not finite")
        expect(call(w=np.array([1.0, np.nan, 1.0])), INV, "negative or not finite")
        expect(call(w=np.array([np.inf, 1.0, 1.0])), INV, "negative or not finite")
        expect(call(Q=2, m=ids(0, 0)), INV, "the same metric twice")
        expect(call(m=ids(3)), INV, "unknown metric")
        expect(call(m=ids(-1)), INV, "unknown metric")
        expect(call(G=_capi.BANK_MAX_GROUPS + 1), UNS,
               "SPFM_BANK_MAX_GROUPS = %d" % _capi.BANK_MAX_GROUPS)
        expect(call(Q=_capi.BANK_MAX_METRICS + 1, m=ids(0, 1, 2, 16, 17)), UNS,
               "SPFM_BANK_MAX_METRICS = %d" % _capi.BANK_MAX_METRICS)
        expect(call(G=0), INV, "G and Q")
        expect(call(Q=0), INV, "G and Q")
        expect(call(y_=None), INV, "NULL")
        expect(call(m=None), INV, "NULL")
        assert call(o=None) == INV
        # valid calls: n = 0 gives zeros, a group without rows gives exact zeros
        small = np.full(2 * F * 3, 7.25)
        assert call(n_=0, y_=None, G=3, Q=2, m=ids(0, 17), o=small) == 0 and (small == 0).all()
        small[:] = 7.25
        assert call(g=ids(0, 2, 0), G=3, o=small) == 0
        tab = small[:F * 3].reshape(F, 3)
        assert (tab[:, 0] == 1.0).all() and (tab[:, 1] == 0).all() and (tab[:, 2] == 0.5).all()
        assert (small[F * 3:] == 7.25).all()  # Q x F x G doubles and no more
    finally:
        eng.close()
