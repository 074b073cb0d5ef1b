"""The host side of cross-validation on one device image (``sparsepoly_amd.model_selection``,
``ModelBank.group_sums``): fold ids, every argument error, the NumPy restatement of the grouped
sums, the assembly of a ``CVResult`` from tables, the cut of the clones into banks.  No GPU: the
device library is made unreachable, so an error that is raised here is raised before it is needed.
"""
import numpy as np
import pytest
import scipy.sparse as sp
from test_explain_host import rows_matrix
from test_ranking_host import fm


@pytest.fixture()
def no_library(monkeypatch):
    """``_capi.load`` and the engine constructor fail loudly: whatever passes did not need them"""
    from sparsepoly_amd import _capi, engine

    def boom(*a, **k):
        raise AssertionError("the device library was asked for")

    monkeypatch.setattr(_capi, "load", boom)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/libspfm_hip.so")
    monkeypatch.setattr(engine.HipEngine, "__init__", boom)


class _NoEngine(object):
    def __getattr__(self, name):
        raise AssertionError("the device was asked for (%s)" % name)

    def close(self):
        pass


def _bank_without_device(ests):
    """a ModelBank whose engine refuses every call: the argument checks must come first"""
    from sparsepoly_amd.bank import ModelBank, _members

    bank = object.__new__(ModelBank)
    bank.estimators, specs, kind = _members(ests)
    bank._d_model = kind[3]
    bank.n_models = len(specs)
    bank._engine = _NoEngine()
    return bank


# ---------------------------------------------------------------- fold_ids
@pytest.mark.parametrize("n,K", [(10, 2), (11, 3), (100, 7), (64, 32), (5, 5)])
@pytest.mark.parametrize("shuffle", [True, False])
def test_fold_sizes(n, K, shuffle):
    from sparsepoly_amd import fold_ids

    f = fold_ids(n, K, shuffle=shuffle, random_state=3)
    assert f.dtype == np.int32 and f.shape == (n,)
    sizes = np.bincount(f, minlength=K)
    assert sizes.shape == (K,) and sizes.max() - sizes.min() <= 1 and sizes.sum() == n


def test_fold_stratification():
    from sparsepoly_amd import fold_ids

    rng = np.random.RandomState(0)
    y = np.array(["a"] * 23 + ["b"] * 7 + ["c"] * 41)[rng.permutation(71)]
    f = fold_ids(71, 5, random_state=1, stratify=y)
    sizes = np.bincount(f, minlength=5)
    assert sizes.max() - sizes.min() <= 1
    for c in "abc":
        per = np.bincount(f[y == c], minlength=5)
        assert per.max() - per.min() <= 1 and per.sum() == (y == c).sum()


def test_fold_determinism_under_a_seed():
    from sparsepoly_amd import fold_ids

    y = np.arange(50) % 2
    for kw in (dict(), dict(stratify=y)):
        a, b = fold_ids(50, 4, random_state=7, **kw), fold_ids(50, 4, random_state=7, **kw)
        c = fold_ids(50, 4, random_state=8, **kw)
        assert (a == b).all() and (a != c).any()
    assert (fold_ids(50, 4, shuffle=False) == fold_ids(50, 4, shuffle=False)).all()


def test_fold_errors():
    from sparsepoly_amd import fold_ids

    with pytest.raises(ValueError, match="n_folds must be >= 2"):
        fold_ids(10, 1)
    with pytest.raises(ValueError, match="at least as many rows"):
        fold_ids(3, 4)
    with pytest.raises(ValueError, match="stratify must hold"):
        fold_ids(10, 2, stratify=np.zeros(9))


# ---------------------------------------------------------------- ModelBank.group_sums: errors
def test_group_sums_argument_errors_come_before_the_device(no_library):
    from sparsepoly_amd import _capi

    ests = [fm(2, k, 12, None, True, seed=k) for k in (2, 3)]
    ests[1].loss = "huber"  # different losses: "loss" must be named
    X = rows_matrix([0, 3, 5, 1, 2, 4], 12, seed=1)
    n = X.shape[0]
    y = np.ones(n)
    g = np.array([0, 1, 2, 0, 1, 2])
    bank = _bank_without_device(ests)
    cases = [
        (dict(y=y[:-1]), "y must be"),
        (dict(y=np.ones((n, 3))), "y must be"),
        (dict(groups=g[:-1]), "groups must be"),
        (dict(groups=g + 0.5), "groups must hold integers"),
        (dict(groups=np.array(["a"] * n)), "groups must hold integers"),
        (dict(groups=g - 1), "negative id"),
        (dict(groups=g, n_groups=2), "n_groups is 2"),
        (dict(groups=g, n_groups=_capi.BANK_MAX_GROUPS + 1), "SPFM_BANK_MAX_GROUPS"),
        (dict(groups=g * 16), "exceed the cap of %d" % _capi.BANK_MAX_GROUPS),
        (dict(n_groups=0), "n_groups must be"),
        (dict(sample_weight=np.ones(n - 1)), "sample_weight has shape"),
        (dict(sample_weight=-y), "negative value"),
        (dict(sample_weight=y * np.nan), "NaN or an infinite"),
        (dict(sample_weight=y * np.inf), "NaN or an infinite"),
        (dict(sample_weight=["a"] * n), "must be numeric"),
        (dict(metrics=("auc",)), "unknown metric"),
        (dict(metrics=()), "at least one"),
        (dict(metrics=("squared", "squared")), "the same metric twice"),
        (dict(metrics=("loss", "squared"), loss="squared"), "the same metric twice"),
        (dict(metrics=("squared", "squared_hinge", "logistic", "abs_error", "sign_error")),
         "SPFM_BANK_MAX_METRICS"),
        (dict(metrics=("loss",)), "different losses"),
        (dict(metrics=("loss",), loss="huber"), "loss must be one of"),
    ]
    for kw, text in cases:
        kw = dict(dict(y=y, metrics=("squared",)), **kw)
        with pytest.raises(ValueError, match=text):
            bank.group_sums(X, **kw)
    with pytest.raises(ValueError, match="negative value"):  # losses(sample_weight=) goes the same way
        bank.losses(X, y, loss="squared", sample_weight=-y)
    with pytest.raises(ValueError, match="X has 11 features"):
        bank.group_sums(X[:, :11], y, metrics=("squared",))
    with pytest.raises(AssertionError, match="the device was asked for"):  # valid: the engine is next
        bank.group_sums(X, y, groups=g, sample_weight=y, metrics=("squared", "sign_error"))


# ---------------------------------------------------------------- restate_group_sums
def _loop_metric(name, p, y):
    import math

    if name == "squared":
        return 0.5 * (p - y) * (p - y)
    if name == "squared_hinge":
        z = 1 - p * y
        return z * z if z > 0 else 0.0
    if name == "logistic":
        z = p * y
        if z > 18:
            return math.exp(-z)
        if z < -18:
            return -z
        return math.log1p(math.exp(-z))
    if name == "abs_error":
        return abs(p - y)
    return 1.0 if (p > 0) != (y > 0) else 0.0


@pytest.mark.parametrize("per_member", [False, True])
def test_restate_group_sums_against_a_double_loop(per_member):
    from sparsepoly_amd.bank import restate_group_sums

    rng = np.random.RandomState(5)
    n, F, G = 57, 3, 4
    sc = rng.randn(n, F) * 12  # logistic: z on both sides of +-18
    sc[0] = 0.0                # a score of 0 is the negative class
    y = np.where(rng.rand(n, F) < 0.5, -1.0, 1.0)
    if not per_member:
        y = y[:, 0]
    w = rng.randint(0, 4, size=n).astype(float)
    g = rng.randint(0, G - 1, size=n)  # group G - 1 has no rows
    names = ["squared", "squared_hinge", "logistic", "abs_error", "sign_error"]
    assert (np.abs(sc * (y if per_member else y[:, None])) > 18).any()
    got = restate_group_sums(sc, y, w, g, G, names)
    want = np.zeros((len(names), F, G))
    for q, name in enumerate(names):
        for i in range(n):
            for f in range(F):
                t = y[i, f] if per_member else y[i]
                want[q, f, g[i]] += w[i] * _loop_metric(name, sc[i, f], t)
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    assert (got[:, :, G - 1] == 0).all()
    assert (got[4] == want[4]).all()  # counts: exact
    wide = restate_group_sums(sc, y, w, g, G, names, wide=True)
    assert wide.dtype == np.longdouble
    np.testing.assert_allclose(wide.astype(float), want, rtol=1e-13, atol=0)
    ones = restate_group_sums(sc, y, None, None, 1, names)
    assert ones.shape == (5, F, 1)
    np.testing.assert_allclose(ones[:, :, 0], restate_group_sums(sc, y, np.ones(n), np.zeros(n), 1,
                                                                 names)[:, :, 0], rtol=0, atol=0)


# ---------------------------------------------------------------- tables -> CVResult
def test_assembly_of_hand_made_tables():
    from sparsepoly_amd.model_selection import CVResult, assemble_cv

    K = 3
    weight = np.array([2.0, 4.0, 8.0])
    held = np.array([0, 1, 2, 0, 1, 2])  # two grid points
    loss = np.array([[6.0, 1.0, 2.0],    # p = 0: test 3, 2, 1 -> mean 2
                     [3.0, 8.0, 5.0],
                     [1.0, 3.0, 8.0],
                     [4.0, 2.0, 6.0],    # p = 1: test 2, 2, 2 -> mean 2: a tie
                     [1.0, 8.0, 3.0],
                     [5.0, 7.0, 16.0]])
    got = assemble_cv({"loss": loss}, weight, held)
    test, train = got["loss"]
    assert (test == [3.0, 2.0, 1.0, 2.0, 2.0, 2.0]).all()
    want_train = [(1.0 + 2.0) / (4.0 + 8.0), (3.0 + 5.0) / (2.0 + 8.0), (1.0 + 3.0) / (2.0 + 4.0),
                  (2.0 + 6.0) / 12.0, (1.0 + 3.0) / 10.0, (5.0 + 7.0) / 6.0]
    assert (train == want_train).all()
    res = CVResult([{"gamma": 1}, {"gamma": 2}], np.zeros(4, dtype=np.int32), K, got, None, {})
    assert res.test_["loss"].shape == (2, K) and (res.test_["loss"][1] == 2.0).all()
    assert (res.mean_test_["loss"] == [2.0, 2.0]).all()
    assert res.std_test_["loss"][1] == 0 and res.std_test_["loss"][0] > 0
    assert res.best_index_ == 0 and res.best_params_ == {"gamma": 1}  # ties: the lowest index
    loss[3:, :] *= 0.5
    res = CVResult([{"gamma": 1}, {"gamma": 2}], None, K, assemble_cv({"loss": loss}, weight, held),
                   None, {})
    assert res.best_index_ == 1
    with pytest.raises(ValueError, match="must be"):
        assemble_cv({"loss": loss[:, :2]}, weight, held)


def test_train_sum_goes_in_ascending_fold_order():
    """three cells whose sum depends on the order: (big + small) + -big against big + (small - big)"""
    from sparsepoly_amd.model_selection import assemble_cv

    big = 2.0 ** 53
    tab = np.array([[0.0, big, 1.0, -big]])
    _, train = assemble_cv({"m": tab}, np.ones(4), np.array([0]))["m"]
    assert train[0] == ((big + 1.0) + -big) / ((1.0 + 1.0) + 1.0) == 0.0
    assert (big + (1.0 + -big)) / 3.0 == 1.0 / 3.0  # what another order would give


# ---------------------------------------------------------------- members -> banks
def test_bank_chunking_of_130_members_of_two_kinds():
    from sparsepoly_amd.model_selection import bank_chunks

    kinds = [("fm", 2, None, i % 2 == 0) for i in range(130)]  # the kinds alternate
    chunks = bank_chunks(kinds, [4] * 130)
    assert chunks == [list(range(0, 128, 2)), [128], list(range(1, 129, 2)), [129]]
    # the component cap cuts too: 10 members of 1000 components, 4 to a bank, in grid order
    chunks = bank_chunks(["a"] * 10, [1000] * 10)
    assert chunks == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert bank_chunks(["a", "b", "a"], [4096, 1, 1]) == [[0], [2], [1]]


def test_kinds_of_real_estimators():
    from sparsepoly_amd import SparseAllSubsetsRegressor, SparseFactorizationMachineRegressor
    from sparsepoly_amd.model_selection import _kind

    a = SparseFactorizationMachineRegressor(degree=3, fit_linear=True)
    b = SparseFactorizationMachineRegressor(degree=3, fit_linear=False)
    assert _kind(a) != _kind(b) and _kind(a) == _kind(SparseFactorizationMachineRegressor(degree=3))
    assert _kind(SparseAllSubsetsRegressor()) == ("all-subsets",)


# ---------------------------------------------------------------- cross_validate_path: errors
class _Split(object):
    def __init__(self, tests):
        self.tests = tests

    def split(self, X, y):
        for t in self.tests:
            yield None, np.asarray(t)


def test_cross_validate_path_errors_come_before_the_device(no_library):
    from sparsepoly_amd import (SparseAllSubsetsRegressor, SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRanker,
                                SparseFactorizationMachineRegressor, _capi, cross_validate_path)
    from sparsepoly_amd.regularizer import L1

    rng = np.random.RandomState(0)
    n = 40
    X = sp.random(n, 8, density=0.4, random_state=rng, format="csr")
    y = rng.randn(n)
    reg = SparseFactorizationMachineRegressor(n_components=2, max_iter=1, random_state=0)

    def bad(text, est=reg, y_=y, **kw):
        kw.setdefault("gamma", [1.0, 0.1])
        with pytest.raises(ValueError, match=text):
            cross_validate_path(est, X, y_, **kw)

    # the grid: fit_path's checks and messages
    with pytest.raises(ValueError, match="at least one parameter sequence"):
        cross_validate_path(reg, X, y)
    bad("same length", beta=[1.0])
    bad("is not a parameter", nonsense=[1, 2])
    # cv
    bad("at least 2 folds", cv=1)
    bad("SPFM_BANK_MAX_GROUPS", cv=_capi.BANK_MAX_GROUPS + 1)
    bad("at least 2 folds", cv=np.zeros(n, dtype=int))
    bad("array of shape", cv=np.zeros(n - 1, dtype=int))
    bad("must be integers", cv=np.arange(n) % 2 + 0.5)
    bad(">= 0", cv=np.arange(n) % 3 - 1)
    bad("SPFM_BANK_MAX_GROUPS", cv=np.arange(n))
    bad("fold 1 has no held-out weight", cv=(np.arange(n) % 2) * 2)  # fold 1 is empty
    bad("in no test set", cv=_Split([range(0, 20), range(20, 39)]))
    bad("in two test sets", cv=_Split([range(0, 21), range(20, 40)]))
    bad("at least 2 folds", cv=_Split([range(0, 40)]))
    # weights
    w = np.ones(n)
    w[np.arange(n) % 2 == 1] = 0.0
    bad("fold 1 has no held-out weight", cv=np.arange(n) % 2, sample_weight=w)
    bad("negative value", sample_weight=-np.ones(n))
    bad("sample_weight has shape", sample_weight=np.ones(n - 1))
    # metrics
    bad("unknown metric", metrics=("auc",))
    bad("picks the smallest mean test 'loss'", metrics=("abs_error",), refit=True)
    bad("the grid varies loss", est=SparseFactorizationMachineClassifier(n_components=2),
        y_=np.sign(y), gamma=[1.0, 1.0], loss=["logistic", "squared_hinge"])
    # what a weighted fit refuses
    bad("distributed=False", est=SparseFactorizationMachineRegressor(distributed=True))
    bad("distributed=False", gamma=[1.0, 1.0], distributed=[False, True])

    class Mine(L1):
        pass

    plug = SparseFactorizationMachineRegressor(regularizer="mine")
    plug._REGULARIZERS = dict(plug._REGULARIZERS, mine=Mine)
    bad("built-in regularizers", est=plug)
    bad("does not take the ranker", est=SparseFactorizationMachineRanker())
    bad("not supported", est=SparseAllSubsetsRegressor(), regularizer=["l1", "nope"], gamma=[1, 1])
    with pytest.raises(TypeError, match="Only binary targets"):
        cross_validate_path(SparseFactorizationMachineClassifier(), X, y, gamma=[1.0])
    # a valid call gets as far as the fits: the library is asked for
    with pytest.raises(AssertionError, match="the device library was asked for"):
        cross_validate_path(reg, X, y, cv=2, gamma=[1.0, 0.1])


def test_integer_cv_is_stratified_for_classifiers_and_seeded(no_library):
    from sparsepoly_amd import SparseFactorizationMachineClassifier, fold_ids
    from sparsepoly_amd.model_selection import _folds_of

    y = np.array([1] * 10 + [0] * 31)
    est = SparseFactorizationMachineClassifier(random_state=4)
    fold, K = _folds_of(3, None, y, 41, est, True)
    assert K == 3 and (fold == fold_ids(41, 3, random_state=4, stratify=y)).all()
    per = np.bincount(fold[y == 1], minlength=3)
    assert per.max() - per.min() <= 1
    fold2, _ = _folds_of(3, None, y, 41, est, False)
    assert (fold2 == fold_ids(41, 3, random_state=4)).all()


def test_clones_carry_the_instance_settings():
    from sparsepoly_amd import SparseFactorizationMachineClassifier
    from sparsepoly_amd.model_selection import _clones

    est = SparseFactorizationMachineClassifier(solver="psgd")
    params, make = _clones(est, dict(gamma=[1.0, 2.0], beta=[3.0, 4.0]))
    assert params == [dict(gamma=1.0, beta=3.0), dict(gamma=2.0, beta=4.0)]
    e = make(params[1])
    assert e.gamma == 2.0 and e.beta == 4.0 and e.solver == "psgd"
    assert "class_weight" not in vars(e) and "adagrad_init" not in vars(e)
    est.class_weight = "balanced"
    est.adagrad_init = 0.5
    e = make(params[0])
    assert e.class_weight == "balanced" and e.adagrad_init == 0.5 and e is not est
