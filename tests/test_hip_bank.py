"""``spfm_bank_*`` and ``sparsepoly_amd.bank.ModelBank`` on the device.  Needs a real MI355X:
``pytest -m gpu``.

Scores are compared with the NumPy restatement ``restate_bank_scores(..., wide=True)``
(``tests/test_bank_host.py`` holds it equal to reference-produced predictions).  The bound comes
from the arithmetic of ``bank_predict_kernel`` (``csrc/spfm_bank.hip.h``) and from no device run.
A score of member f is a sum of signed monomials; one of them goes through at most

    N = n_i + 2 M + 1 + k_f + 2            (all-subsets: 3 n_i + 1 + k_f + 2)

roundings (``n_i`` the stored entries of the augmented row, ``M`` the degree, ``k_f`` the member's
components):
  * the DP ``a[t] += a[t-1] (p x)``: one per factor ``p x``, one per multiplication by it, and one
    per addition of the recurrence, of which the monomial rides at most one per entry:
    ``n_i + 2 M``; the all-subsets product ``a *= 1 + x p`` rounds three times per entry, and
    every monomial of its expansion goes through all of them: ``3 n_i``;
  * the product with ``lams``: 1;
  * the component sum: lane f adds its member's terms one after the other in the member's own
    component order, so a term goes through at most ``k_f`` additions;
  * ``(B_0 + lin) + B_1``: 2 (a monomial of the linear term: ``x w``, ``n_i`` additions, these 2).
So ``|device - exact| <= (N + 2) 2^-53 S_hat``, ``S_hat`` the sum of the monomials' magnitudes:
the output of ``abs_model`` on ``|X|`` in ``longdouble``; the 2 covers the second-order terms and
the ``longdouble`` reference.  Nothing in N depends on the other members, the member's position,
the slabs or the grid, as nothing in the kernel does.

Loss sums: per row the loss of the computed score differs from the loss of the exact one by the
score's bound times the loss's slope, plus the loss's own roundings (``_loss_terms``); a row's
loss then goes through the butterfly and the four waves of its block (10 additions), the finish's
strided sum over the P blocks (``ceil(P / 256)``) and its butterfly and waves (10):
``N_sum = 20 + ceil(P / 256)``, error ``(N_sum + 2) 2^-53 sum_i loss_i``.  The reference applies
the project's own piecewise definition of the loss (``loss_dev``) in ``longdouble``.

Weighted mean: ``sum_f |w_f| bound_if + (F + 3) 2^-53 sum_f |w_f| S_hat_if`` (one product, at most
F additions).

Orders are exact.  Where the device argmax is compared with NumPy's on the restated scores, the
NumPy side first asserts, before the device is touched, that best and runner-up are at least
``CLEAR * max|score|`` apart on every row; the seeds pass that on the CPU and no row is left out.
Each case prints its largest error as a fraction of its bound before asserting.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
from test_explain_host import COMBOS, rows_matrix
from test_ranking_host import abs_model, all_subsets, fm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CLEAR = 1e-9
LENGTHS = [0, 1, 2, 63, 64, 65, 130, 700, 5, 0]  # empty first and last row
D = 800
SMALL = [0, 1, 2, 5, 9, 0]
KS = (1, 30, 64, 65, 130)  # member boundaries inside, on and across the chunks of 64


def _reference(ests, X):
    """(exact scores, bound, S_hat), all (n, F) longdouble, all NumPy"""
    from sparsepoly_amd.bank import _members, _prepare, restate_bank_scores

    _, specs, (degree, _, _, d_model) = _members(ests)
    want = restate_bank_scores(ests, X, wide=True)
    S = restate_bank_scores([abs_model(e) for e in ests], abs(sp.csr_matrix(X)), wide=True)
    n_i = np.diff(_prepare(ests[0], X, d_model).indptr).astype(np.longdouble)[:, None]
    k_f = np.array([s[3].shape[1] for s in specs], dtype=np.longdouble)[None, :]
    N = (3 * n_i if degree == -1 else n_i + 2 * degree) + 1 + k_f + 2
    return want, (N + 2) * U * S, S


def _check(got, want, bound, what):
    assert want.dtype == np.longdouble and got.shape == want.shape and got.dtype == np.float64
    err = np.abs(got.astype(np.longdouble) - want)
    ok = bound > 0
    frac = float((err[ok] / bound[ok]).max(initial=0.0))
    print("%s: largest error %.3g of its bound" % (what, frac))
    assert (err <= bound).all(), (what, frac)


def _check_bank(ests, X, what, **kw):
    from sparsepoly_amd import ModelBank

    want, bound, _ = _reference(ests, X)
    with ModelBank(ests, **kw) as bank:
        got = bank.decision_function(X)
        again = bank.decision_function(X)
    _check(got, want, bound, what)
    assert (got == again).all()
    return got


@pytest.fixture(scope="module")
def mixed():
    """one bank of members with k in KS (degree 3, two blocks, linear term) over the long rows,
    its reference computed once"""
    ests = [fm(3, k, D, "explicit", True, seed=70 + k) for k in KS]
    X = rows_matrix(LENGTHS, D, seed=7)
    return ests, X, _reference(ests, X)


# ---------------------------------------------------------------- 1. scores
@pytest.mark.parametrize("degree,fl,lin", COMBOS)
def test_scores_equal_the_restatement(degree, fl, lin):
    ests = [fm(degree, k, 12, fl, lin, seed=10 * degree + k) for k in (5, 1, 7)]
    _check_bank(ests, rows_matrix(SMALL, 12, seed=degree), "degree %d %s %d" % (degree, fl, lin))


def test_mixed_component_counts_long_rows_two_blocks(mixed):
    """degree 3 'explicit' (the order-2 block too), k = 1, 30, 64, 65, 130 in one bank: S = 290,
    member boundaries at 1, 31, 95, 160; rows of 0 .. 700 entries (the staging holds 128)"""
    from sparsepoly_amd import ModelBank

    ests, X, (want, bound, _) = mixed
    with ModelBank(ests) as bank:
        got = bank.decision_function(X)
        assert bank.info()["S"] == sum(KS) and bank.info()["n_models"] == len(KS)
        assert bank.info()["launches"] == 2 and bank.info()["slabs"] == 1
        assert bank.info()["resident_bytes"] >= 8 * (2 * D * sum(KS) + sum(KS) + D * len(KS))
    _check(got, want, bound, "mixed k")
    assert (got[0] == 0).all() and (got[-1] == 0).all()  # empty rows: the base value


@pytest.mark.parametrize("degree", [2, 4, 5, 6])
def test_mixed_component_counts_other_degrees(degree):
    ests = [fm(degree, k, D, None, True, seed=degree + k) for k in KS[::-1]]
    _check_bank(ests, rows_matrix(LENGTHS, D, seed=degree), "degree %d, mixed k" % degree)


@pytest.mark.parametrize("F", [1, 2, 3, 64])
def test_number_of_members(F):
    ests = [fm(2, 30, D, None, True, seed=200 + f) for f in range(F)]
    _check_bank(ests, rows_matrix(LENGTHS, D, seed=F), "F = %d" % F)


def test_all_subsets_bank():
    ests = [all_subsets(k, 60, seed=k) for k in (3, 64, 30)]
    X = rows_matrix([0, 1, 7, 60, 3], 60, seed=4)
    got = _check_bank(ests, X, "all-subsets")
    for f, e in enumerate(ests):  # an empty row: the product is 1 for every component
        assert got[0, f] == e.lams_.sum()  # (a sum of +-1: exact)


def test_classifier_bank():
    from sparsepoly_amd import SparseAllSubsetsClassifier, SparseFactorizationMachineClassifier

    X = rows_matrix(SMALL + [12], 12, seed=8)
    _check_bank([fm(3, k, 12, "augment", True, seed=k, cls=SparseFactorizationMachineClassifier)
                 for k in (4, 9)], X, "classifiers")
    _check_bank([all_subsets(k, 12, seed=k, cls=SparseAllSubsetsClassifier) for k in (4, 9)], X,
                "all-subsets classifiers")


# ---------------------------------------------------------------- 2. what a score may depend on
def test_a_column_does_not_depend_on_the_other_members(mixed):
    from sparsepoly_amd import ModelBank

    ests, X, _ = mixed
    A, B, Cm = ests[1], ests[3], ests[4]  # k = 30, 65, 130: B straddles chunks in every position
    cols = []
    for members, at in (([A, B, Cm], 1), ([B], 0), ([Cm, B], 1)):
        with ModelBank(members) as bank:
            cols.append(bank.decision_function(X)[:, at])
    assert (cols[0] == cols[1]).all() and (cols[1] == cols[2]).all()
    assert np.abs(cols[0]).max() > 0


def test_partition_independence(mixed):
    """slabs of at most 6 stored entries: edges on the empty first row, between rows, every long
    row alone in its slab; scores, argmax and mean are bit-identical to the default's"""
    from sparsepoly_amd import ModelBank

    ests, X, _ = mixed
    wts = np.linspace(-1, 2, len(ests))
    with ModelBank(ests) as bank:
        whole = bank.decision_function(X), bank.argmax(X), bank.mean(X, wts)
        assert bank.info()["slabs"] == 1
        bank.set_partition(6)
        parts = bank.decision_function(X), bank.argmax(X), bank.mean(X, wts)
        assert bank.info()["slabs"] > 1
        assert bank.info()["launches"] == 2 * bank.info()["slabs"]
        bank.set_partition(0)
        assert (bank.decision_function(X) == whole[0]).all() and bank.info()["slabs"] == 1
    assert (parts[0] == whole[0]).all() and (parts[2] == whole[2]).all()
    for a, b in zip(parts[1], whole[1]):
        assert (a == b).all()


# ---------------------------------------------------------------- 3. argmax
def test_argmax_equals_numpy_on_the_device_scores():
    """degree 3 'augment' with a linear term: the dummy column gives every member its own base
    value, so the empty rows have distinct scores too"""
    from sparsepoly_amd import ModelBank

    ests = [fm(3, k, D, "augment", True, seed=80 + k) for k in KS]
    X = rows_matrix(LENGTHS, D, seed=7)
    want, _, _ = _reference(ests, X)
    # NumPy side first: the exact best and runner-up are clearly apart on every row
    srt = np.sort(want, axis=1)
    assert (srt[:, -1] - srt[:, -2] >= CLEAR * np.abs(want).max()).all()
    with ModelBank(ests) as bank:
        sc = bank.decision_function(X)
        idx, best, runner = bank.argmax(X)
    assert idx.dtype == np.int32 and idx.shape == best.shape == runner.shape == (X.shape[0],)
    assert (idx == sc.argmax(axis=1)).all()
    assert (best == sc.max(axis=1)).all()
    assert (runner == np.sort(sc, axis=1)[:, -2]).all()
    assert (idx == want.argmax(axis=1)).all()
    # empty rows: the scores are the base values, here the dummy column's linear weights
    base = np.array([e.w_[0] for e in ests])  # add_dummy_feature puts it first
    assert (sc[0] == base).all() and (sc[-1] == base).all()
    assert idx[0] == idx[-1] == base.argmax()


def test_argmax_of_all_equal_scores_is_the_first_member(mixed):
    from sparsepoly_amd import ModelBank

    ests, X, _ = mixed
    with ModelBank(ests) as bank:
        idx, best, runner = bank.argmax(X)
    for i in (0, -1):  # empty rows, no dummy column: every score is 0
        assert idx[i] == 0 and best[i] == 0 and runner[i] == 0


def test_argmax_ties_and_a_single_member():
    from sparsepoly_amd import ModelBank

    X = rows_matrix(LENGTHS, D, seed=9)
    a, b = fm(2, 65, D, None, True, seed=1), fm(2, 30, D, None, True, seed=2)
    with ModelBank([b, a, a]) as bank:
        sc = bank.decision_function(X)
        idx, best, runner = bank.argmax(X)
    assert (sc[:, 1] == sc[:, 2]).all()  # the same member twice: an exact tie
    assert not (idx == 2).any() and (idx == 1).any()
    wins = idx == 1
    assert (runner[wins] == best[wins]).all()
    with ModelBank([a]) as bank:
        idx, best, runner = bank.argmax(X)
        assert (best == bank.decision_function(X)[:, 0]).all()
    assert (idx == 0).all() and np.isneginf(runner).all()


# ---------------------------------------------------------------- 4. losses
def _loss_wide(loss, p, y):
    """the project's loss (``loss_dev``: the reference's piecewise definitions) in longdouble"""
    p, y = p.astype(np.longdouble), y.astype(np.longdouble)
    if loss == "squared":
        return 0.5 * (p - y) ** 2
    if loss == "squared_hinge":
        return np.maximum(1 - p * y, 0) ** 2
    z = p * y
    zc = np.clip(z, -18, 18)
    return np.where(z > 18, np.exp(-z), np.where(z < -18, -z, np.log1p(np.exp(-zc))))


def _loss_terms(loss, p, y, b):
    """per (row, member): how far the loss of a score within ``b`` of ``p`` can be from
    ``loss(p, y)``, plus the roundings of the loss's own evaluation"""
    p, y, b = np.abs(p), np.abs(y), b.astype(np.longdouble)
    if loss == "squared":  # (p - y)^2 / 2: a subtraction and a product (the half is exact)
        r = p + y
        return b * (r + b / 2) + 3 * U * 0.5 * (r + b) ** 2
    if loss == "squared_hinge":  # z = 1 - p y, z^2: slope 2 |y| |z|; z is off by u (|p y| + |z|)
        z = 1 + p * y
        return b * y * (2 * z + y * b) + U * (2 * z * (p * y + z) + z * z) * 2
    # logistic: slope <= |y|.  z = p y rounds once (u |z|, slope 1).  exp and log taken within
    # 2 ulp = 4 u: the argument 1 + e is off by at most 4 u e + u (1 + e) <= 5 u (1 + e), which the
    # log turns into 5 u; its own error is 4 u loss <= 4 u (|z| + 1).  The outer branches (exp(-z),
    # -z) stay below that.
    return b * y + U * (5 * p * y + 9) * 2


def _loss_case():
    ests = [fm(2, k, 40, None, True, seed=300 + k) for k in (3, 30, 65)]
    for e in ests:  # moderate scores: the logistic loss away from its branches at |z| = 18
        e.P_ *= 0.5
        e.w_ *= 0.3
    X = rows_matrix([0, 1, 5, 40, 12, 7, 3, 9] * 75, 40, seed=11)  # 600 rows: 3 blocks of 256
    rng = np.random.RandomState(12)
    y = np.where(rng.rand(X.shape[0]) < 0.5, -1.0, 1.0)
    Y = np.where(rng.rand(X.shape[0], len(ests)) < 0.5, -1.0, 1.0)
    return ests, X, y, Y, _reference(ests, X)


@pytest.fixture(scope="module")
def loss_case():
    return _loss_case()


@pytest.mark.parametrize("loss", ["squared", "squared_hinge", "logistic"])
def test_loss_sums(loss_case, loss):
    from sparsepoly_amd import ModelBank

    ests, X, y, Y, (want, bound, _) = loss_case
    n = X.shape[0]
    if loss == "logistic":  # no score within reach of the branch points
        for t in (y[:, None], Y):
            assert (np.abs(np.abs(want * t) - 18) > 1e-6).all()
    with ModelBank(ests) as bank:
        for targets, what in ((y, "shared y"), (Y, "per-member Y")):
            t2 = targets[:, None] if targets.ndim == 1 else targets
            exact = _loss_wide(loss, want, t2)
            P = -(-n // 256)
            tol = (_loss_terms(loss, want, t2, bound).sum(axis=0)
                   + (20 + -(-P // 256) + 2) * U * exact.sum(axis=0))
            got = bank.losses(X, targets, loss=loss)
            assert got.shape == (len(ests),) and got.dtype == np.float64
            _check(got, exact.sum(axis=0), tol, "%s, %s" % (loss, what))
            assert (bank.losses(X, targets, loss=loss) == got).all()  # run to run
            assert (bank.losses(X, targets, loss=loss, mean=True) == got / n).all()
        bank.set_partition(50)  # many slabs: another partition of the rows, the same bound
        P = n  # at most one block per row
        got = bank.losses(X, y, loss=loss)
        assert bank.info()["slabs"] > 10
        exact = _loss_wide(loss, want, y[:, None])
        tol = (_loss_terms(loss, want, y[:, None], bound).sum(axis=0)
               + (20 + -(-P // 256) + 2) * U * exact.sum(axis=0))
        _check(got, exact.sum(axis=0), tol, "%s, slabs of 50 entries" % loss)


def test_default_loss_and_its_errors(loss_case):
    from sparsepoly_amd import ModelBank, SparseFactorizationMachineClassifier

    ests, X, y, Y, _ = loss_case
    clf = [fm(2, 3, 40, None, True, seed=s, cls=SparseFactorizationMachineClassifier)
           for s in (1, 2)]
    clf[1].loss = "logistic"
    with ModelBank(ests) as bank:  # regressors: their common loss is 'squared'
        assert (bank.losses(X, y) == bank.losses(X, y, loss="squared")).all()
        with pytest.raises(ValueError, match="y must be"):
            bank.losses(X, y[:-1])
        with pytest.raises(ValueError, match="y must be"):
            bank.losses(X, Y[:, :2])
        with pytest.raises(ValueError, match="loss must be one of"):
            bank.losses(X, y, loss="huber")
    with ModelBank(clf) as bank:
        with pytest.raises(ValueError, match="different losses"):
            bank.losses(X, y)
        assert bank.losses(X, y, loss="logistic").shape == (2,)


# ---------------------------------------------------------------- 5. mean
def test_weighted_mean(mixed):
    from sparsepoly_amd import ModelBank

    ests, X, (want, bound, S) = mixed
    F = len(ests)
    with ModelBank(ests) as bank:
        for wts in (None, np.array([0.5, -2.0, 0.0, 1.25, 3.0])):
            w = np.full(F, 1.0 / F) if wts is None else wts
            wl = np.abs(w).astype(np.longdouble)[None, :]
            exact = (want * w.astype(np.longdouble)[None, :]).sum(axis=1)
            tol = (wl * bound).sum(axis=1) + (F + 3) * U * (wl * S).sum(axis=1)
            got = bank.mean(X, wts)
            assert got.shape == (X.shape[0],)
            _check(got, exact, tol, "mean, %s weights" % ("default" if wts is None else "given"))
        for bad in (np.ones(F - 1), np.ones(F + 1), np.ones((F, 1))):
            with pytest.raises(ValueError, match="weights must be"):
                bank.mean(X, bad)


# ---------------------------------------------------------------- 6. inputs and precision
def test_dense_csc_and_messy_input():
    from sparsepoly_amd import ModelBank

    ests = [fm(3, k, 40, "augment", True, seed=k) for k in (30, 5)]
    X = rows_matrix([0, 3, 40, 17, 0], 40, seed=5)
    want, bound, _ = _reference(ests, X)
    messy = _messy(X)
    assert not messy.has_sorted_indices and messy.nnz == 2 * X.nnz
    before = messy.data.copy(), messy.indices.copy(), messy.indptr.copy()
    with ModelBank(ests) as bank:
        for form in (X.tocsc(), X.toarray(), messy):
            _check(bank.decision_function(form), want, bound, type(form).__name__)
    for a, b in zip(before, (messy.data, messy.indices, messy.indptr)):
        assert (a == b).all()
    assert not messy.has_canonical_format


def _messy(X):
    """the rows of X with every entry stored twice (two halves of it: their sum is exact), the
    columns of a row in descending order"""
    data, idx, ptr = [], [], [0]
    for i in range(X.shape[0]):
        lo, hi = X.indptr[i], X.indptr[i + 1]
        c, v = X.indices[lo:hi][::-1], X.data[lo:hi][::-1]
        idx += [c, c]
        data += [0.5 * v, 0.5 * v]
        ptr.append(ptr[-1] + 2 * (hi - lo))
    return sp.csr_matrix((np.concatenate(data), np.concatenate(idx).astype(np.int32),
                          np.array(ptr, dtype=np.int64)), shape=X.shape)


def test_f32_storage_sees_the_same_inputs():
    """precision='f32': x is rounded to float32 first, so both sides see the same inputs; the
    arithmetic is f64 for either storage type and the bound is unchanged"""
    ests = [fm(3, k, D, "explicit", True, seed=6 + k) for k in (30, 65)]
    X = rows_matrix(LENGTHS, D, seed=6, f32=True)
    _check_bank(ests, X, "f32", precision="f32")
    for e in ests:
        e.precision = "f32"
    _check_bank(ests, X, "f32 from the members")


# ---------------------------------------------------------------- 7. the C entry points' errors
def test_entry_point_errors():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    lib = eng._lib
    d, F, k = 6, 2, 3
    koff = np.array([0, k, 2 * k], dtype=np.int32)
    deg = np.array([2], dtype=np.int32)
    Pt = np.zeros((1, d, 2 * k))
    lams = np.ones(2 * k)
    w = np.zeros((d, F))
    X = rows_matrix([2, 0, 3], d, seed=1)
    ip, ii, dd = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data
    out = np.zeros((3, F))
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    i32, i64, f64 = C.c_int32, C.c_int64, C.c_double

    def expect(rc, code, text):
        msg = lib.spfm_last_error(eng._h).decode()
        assert rc == code and text in msg, (rc, msg)

    def scores(n=3, dd_=d, ip_=ip, ii_=ii, data=p(dd, f64), o=p(out, f64)):
        return lib.spfm_bank_scores(eng._h, n, dd_, p(ip_, i64), p(ii_, i32), data, o)

    def bank_set(F_=F, koff_=koff, nb=1, deg_=deg, d_=d, Pt_=p(Pt, f64), lams_=p(lams, f64)):
        return lib.spfm_bank_set(eng._h, d_, F_, p(koff_, i32), nb, p(deg_, i32), Pt_, lams_,
                                 p(w, f64))

    try:
        expect(scores(), _capi.SPFM_ERR_INVALID, "no bank set")
        expect(bank_set(Pt_=None), _capi.SPFM_ERR_INVALID, "NULL")
        expect(bank_set(lams_=None), _capi.SPFM_ERR_INVALID, "NULL")
        expect(bank_set(F_=0), _capi.SPFM_ERR_INVALID, "at least one model")
        expect(bank_set(d_=0), _capi.SPFM_ERR_INVALID, "d must be")
        expect(bank_set(nb=3), _capi.SPFM_ERR_INVALID, "n_blocks")
        expect(bank_set(koff_=np.array([0, 3, 3], dtype=np.int32)), _capi.SPFM_ERR_INVALID,
               "koff must increase")
        expect(bank_set(koff_=np.array([1, 3, 6], dtype=np.int32)), _capi.SPFM_ERR_INVALID,
               "koff[0]")
        expect(bank_set(deg_=np.array([7], dtype=np.int32)), _capi.SPFM_ERR_UNSUPPORTED, "degree")
        # above the caps: refused by name before anything is read or copied
        many = np.arange(_capi.BANK_MAX_MODELS + 2, dtype=np.int32)
        expect(bank_set(F_=_capi.BANK_MAX_MODELS + 1, koff_=many), _capi.SPFM_ERR_UNSUPPORTED,
               "SPFM_BANK_MAX_MODELS = %d" % _capi.BANK_MAX_MODELS)
        wide = np.array([0, _capi.BANK_MAX_COMPONENTS + 1], dtype=np.int32)
        expect(bank_set(F_=1, koff_=wide), _capi.SPFM_ERR_UNSUPPORTED,
               "SPFM_BANK_MAX_COMPONENTS = %d" % _capi.BANK_MAX_COMPONENTS)
        expect(scores(), _capi.SPFM_ERR_INVALID, "no bank set")  # a refused set leaves no bank
        assert bank_set() == 0
        assert scores() == 0
        expect(scores(dd_=d + 1), _capi.SPFM_ERR_INVALID, "the bank has d = %d" % d)
        expect(scores(o=None), _capi.SPFM_ERR_INVALID, "NULL output")
        expect(scores(data=None), _capi.SPFM_ERR_INVALID, "NULL array")
        bad = ii.copy()
        bad[-1] = d
        expect(scores(ii_=bad), _capi.SPFM_ERR_INVALID, "column index out of range")
        expect(scores(ip_=ip + 1), _capi.SPFM_ERR_INVALID, "indptr[0]")
        expect(scores(ip_=ip[::-1].copy() - ip[-1] + 0), _capi.SPFM_ERR_INVALID, "indptr")
        y = np.ones(3)
        lo = np.zeros(F)
        args = (eng._h, 3, d, p(ip, i64), p(ii, i32), p(dd, f64))
        expect(lib.spfm_bank_losses(*args, 7, p(y, f64), 0, p(lo, f64)), _capi.SPFM_ERR_INVALID,
               "unknown loss")
        expect(lib.spfm_bank_losses(*args, 0, None, 0, p(lo, f64)), _capi.SPFM_ERR_INVALID, "NULL")
        expect(lib.spfm_bank_argmax(*args, None, p(y, f64), p(y, f64)), _capi.SPFM_ERR_INVALID,
               "NULL output")
        expect(lib.spfm_bank_mean(*args, None, None), _capi.SPFM_ERR_INVALID, "NULL output")
        expect(lib.spfm_bank_set_partition(eng._h, -1), _capi.SPFM_ERR_INVALID, "slab_nnz")
        assert scores(n=0, o=None) == 0  # n = 0 is valid and writes nothing
        assert lib.spfm_bank_losses(eng._h, 0, d, p(ip, i64), None, None, 0, None, 0,
                                    p(lo, f64)) == 0 and (lo == 0).all()
        assert eng.bank_info()["resident_bytes"] > 0
        eng.bank_release()
        assert eng.bank_info()["resident_bytes"] == 0 and eng.bank_info()["S"] == 0
        expect(scores(), _capi.SPFM_ERR_INVALID, "no bank set")
    finally:
        eng.close()
