"""The host side of ``ModelBank.group_auc`` and of ``cross_validate_path(rank_metrics=)``: the
NumPy restatement ``restate_group_auc`` against two yardsticks that are not this project's code
(an O(n^2) loop over the pairs, ``sklearn.metrics.roc_auc_score``), every new argument error, and
why the training AUC of a fold cannot be assembled from per-fold tables.  No GPU.

Weighted bound.  With u = 2^-53, every quantity a sum or product of non-negative numbers: a class
weight or a running weight of the negatives is a sum of at most n terms (relative error at most
(n - 1) u in any order); ``C[lo] + C[hi]`` adds one rounding, the product with ``w_p`` one, the
halving none, the sum over the positives at most n - 1: the numerator is within (2n + 1) u, the
denominator ``W_pos W_neg`` within (2n - 1) u, the quotient adds one.  (4n + 16) u covers both
sides of a comparison's second-order terms and the conversion of a wider reference.
"""
import numpy as np
import pytest
import scipy.sparse as sp
from test_explain_host import rows_matrix
from test_model_selection_host import _bank_without_device, no_library  # noqa: F401
from test_ranking_host import fm

N, F, G = 60, 3, 4
U53 = 2.0 ** -53


def _loop(s, pos, w, rows):
    """the O(n^2) yardstick on the rows ``rows``: (2 * numerator, W_pos, W_neg) in Python numbers,
    the scores compared as numbers (so -0.0 == +0.0)"""
    idx = np.flatnonzero(rows)
    two = wp = wn = 0
    for i in idx:
        if pos[i]:
            wp += w[i]
        else:
            wn += w[i]
    for p in idx:
        if not pos[p]:
            continue
        for q in idx:
            if pos[q]:
                continue
            if s[q] < s[p]:
                two += 2 * w[p] * w[q]
            elif s[q] == s[p]:
                two += w[p] * w[q]
    return two, wp, wn


@pytest.fixture(scope="module")
def case():
    rng = np.random.RandomState(5)
    scores = rng.randn(N, F)
    scores[:, 0] = np.round(scores[:, 0] * 2) / 2           # many ties
    scores[:, 1] = np.where(rng.rand(N) < 0.5, -0.0, 0.0)    # one run of both zeros
    scores[::7, 2] = scores[3, 2]                            # a tie run inside distinct scores
    y = np.where(rng.rand(N) < 0.4, 1.0, -1.0)
    Y = np.where(rng.rand(N, F) < 0.5, 1.0, -1.0)
    g = rng.randint(0, 3, size=N)                            # group 3 holds no row
    y[g == 2] = -1.0                                         # group 2 holds no positive
    Y[g == 2] = -1.0
    w = rng.randint(0, 4, size=N).astype(np.double) * 0.75   # zero weights
    sets = np.zeros((F, 5, G), dtype=bool)
    sets[:, 0, 0] = True                                     # one group
    sets[:, 1, [0, 1]] = True                                # a union
    sets[:, 2, 2] = True                                     # no positives: NaN
    sets[:, 3, 3] = True                                     # empty
    for f in range(F):
        sets[f, 4] = np.arange(G) != f                       # a complement, per member
    return scores, y, Y, g, w, sets


@pytest.mark.parametrize("per_member", [False, True])
def test_unweighted_integers_equal_the_loop(case, per_member):
    from sparsepoly_amd.bank import restate_group_auc

    scores, y, Y, g, w, sets = case
    t = Y if per_member else y
    got = restate_group_auc(scores, t, None, g, G, sets)
    assert got["pairs"].dtype == np.int64 and got["pairs"].shape == (F, 5, 3)
    ones = np.ones(N, dtype=int)
    for f in range(F):
        pos = (t[:, f] if per_member else t) > 0
        for u in range(5):
            two, npos, nneg = _loop(scores[:, f], pos, ones, sets[f, u][g])
            assert tuple(got["pairs"][f, u]) == (two, npos, nneg)
            assert got["pos_weight"][f, u] == npos and got["neg_weight"][f, u] == nneg
            if npos * nneg == 0:
                assert np.isnan(got["auc"][f, u])
            else:
                assert got["auc"][f, u] == float(two) / (2.0 * float(npos) * float(nneg))
    assert np.isnan(got["auc"][:, 2]).all() and (got["pairs"][:, 2, 1] == 0).all()
    assert (got["pairs"][:, 2, 2] > 0).all()                  # the counts are reported
    assert np.isnan(got["auc"][:, 3]).all() and (got["pairs"][:, 3] == 0).all()
    # -0.0 against +0.0: one run, every pair tied
    assert (got["auc"][1, :2] == 0.5).all()


@pytest.mark.parametrize("wide", [False, True])
def test_weighted_values_are_within_the_bound_of_the_loop(case, wide):
    from fractions import Fraction

    from sparsepoly_amd.bank import restate_group_auc

    scores, y, Y, g, w, sets = case
    rng = np.random.RandomState(6)
    for wt in (w, rng.rand(N) + 0.5):
        got = restate_group_auc(scores, Y, wt, g, G, sets, wide=wide)
        assert "pairs" not in got
        exact_w = [Fraction(float(v)) for v in wt]
        for f in range(F):
            for u in range(5):
                two, wp, wn = _loop(scores[:, f], Y[:, f] > 0, exact_w, sets[f, u][g])
                assert abs(got["pos_weight"][f, u] - float(wp)) <= N * U53 * float(wp)
                assert abs(got["neg_weight"][f, u] - float(wn)) <= N * U53 * float(wn)
                if wp * wn == 0:
                    assert np.isnan(got["auc"][f, u])
                    continue
                exact = two / (2 * wp * wn)  # a Fraction: no rounding at all
                err = abs(Fraction(float(got["auc"][f, u])) - exact)
                assert err <= Fraction((4 * N + 16) * U53) * exact, (f, u, float(err / exact))


def test_against_sklearn(case):
    from sklearn.metrics import roc_auc_score

    from sparsepoly_amd.bank import restate_group_auc

    scores, y, Y, g, w, sets = case
    s = scores + 0.0
    for wt in (None, w):
        got = restate_group_auc(scores, Y, wt, g, G, sets)["auc"]
        for f in range(F):
            for u in (0, 1, 4):
                rows = sets[f, u][g]
                want = roc_auc_score(Y[rows, f] > 0, s[rows, f],
                                     sample_weight=None if wt is None else wt[rows])
                # sklearn integrates the curve by trapezoids in double: other sums of the same
                # non-negative terms, so the module's bound holds between the two
                assert abs(got[f, u] - want) <= (4 * N + 16) * U53 * want


def test_sets_forms(case):
    from sparsepoly_amd.bank import restate_group_auc

    scores, y, Y, g, w, sets = case
    default = restate_group_auc(scores, y, None, g, G, None)
    eye = restate_group_auc(scores, y, None, g, G, np.eye(G, dtype=bool))
    assert default["pairs"].shape == (F, G, 3) and (default["pairs"] == eye["pairs"]).all()
    shared = restate_group_auc(scores, y, w, g, G, sets[0])
    full = restate_group_auc(scores, y, w, g, G, np.broadcast_to(sets[0], (F, 5, G)))
    assert np.array_equal(shared["auc"], full["auc"], equal_nan=True)
    none = restate_group_auc(scores, y, None, None, 1, None)
    assert none["pairs"].shape == (F, 1, 3) and (none["pairs"][:, 0, 1] == (y > 0).sum()).all()


def test_group_auc_argument_errors_come_before_the_device(no_library):  # noqa: F811
    from sparsepoly_amd import _capi

    ests = [fm(2, k, 12, None, True, seed=k) for k in (2, 3)]
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
        (dict(groups=g - 1), "negative id"),
        (dict(groups=g, n_groups=2), "n_groups is 2"),
        (dict(groups=g, n_groups=_capi.BANK_MAX_GROUPS + 1), "SPFM_BANK_MAX_GROUPS"),
        (dict(n_groups=0), "n_groups must be"),
        (dict(sample_weight=np.ones(n - 1)), "sample_weight has shape"),
        (dict(sample_weight=-y), "negative value"),
        (dict(sample_weight=y * np.nan), "NaN or an infinite"),
        (dict(sample_weight=["a"] * n), "must be numeric"),
        (dict(groups=g, sets=np.ones((2, 4), dtype=bool)), "sets must be"),
        (dict(groups=g, sets=np.ones((3, 2, 3), dtype=bool)), "sets must be"),
        (dict(groups=g, sets=np.ones(3, dtype=bool)), "sets must be"),
        (dict(groups=g, sets=np.ones((0, 3), dtype=bool)), "at least one set"),
        (dict(groups=g, sets=np.full((2, 3), 2)), "sets must be boolean"),
        (dict(groups=g, sets=np.ones((_capi.BANK_MAX_SETS + 1, 3), dtype=bool)),
         "SPFM_BANK_MAX_SETS"),
    ]
    for kw, text in cases:
        kw = dict(dict(y=y), **kw)
        with pytest.raises(ValueError, match=text):
            bank.group_auc(X, **kw)
    # a valid call reaches the device
    with pytest.raises(AssertionError, match="the device was asked for"):
        bank.group_auc(X, y, groups=g, sets=np.ones((2, 3), dtype=bool))
    # group_sums keeps refusing the name: auc is no sum over rows
    with pytest.raises(ValueError, match="unknown metric"):
        bank.group_sums(X, y, metrics=("auc",))


def test_set_masks():
    from sparsepoly_amd.bank import _set_masks

    assert _set_masks(None, 3, 4) is None
    s = np.zeros((2, 32), dtype=bool)
    s[0, [0, 31]] = True
    s[1, 5] = True
    m = _set_masks(s, 3, 32)
    assert m.dtype == np.uint32 and m.shape == (3, 2)
    assert (m[:, 0] == (1 << 31) + 1).all() and (m[:, 1] == 32).all()


def test_rank_metrics_errors_come_before_the_device(no_library):  # noqa: F811
    from sparsepoly_amd import (SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor, cross_validate_path)

    rng = np.random.RandomState(0)
    n = 40
    X = sp.random(n, 8, density=0.4, random_state=rng, format="csr")
    y = np.where(np.arange(n) % 4 == 0, 1, 0)
    clf = SparseFactorizationMachineClassifier(n_components=2, max_iter=1, random_state=0)
    reg = SparseFactorizationMachineRegressor(n_components=2, max_iter=1, random_state=0)

    def bad(text, est=clf, y_=y, **kw):
        kw.setdefault("gamma", [1.0, 0.1])
        with pytest.raises(ValueError, match=text):
            cross_validate_path(est, X, y_, **kw)

    bad("unknown rank metric", rank_metrics=("ap",))
    bad("unknown rank metric", rank_metrics=("auc", 3))
    bad("the same metric twice", rank_metrics=("auc", "auc"))
    bad("need a classifier", est=reg, y_=rng.randn(n), rank_metrics=("auc",))
    bad("select must be", select="auc")
    bad("select must be", rank_metrics=("auc",), select="sign_error")
    bad("select='loss'", metrics=("sign_error",), select="loss")
    bad("picks the smallest mean test 'loss'", metrics=("sign_error",), rank_metrics=("auc",),
        refit=True)
    bad("unknown metric", metrics=("auc",))  # the sums keep refusing the name
    # a fold without a class (every training complement is a union of folds: covered with them)
    fold = np.arange(n) % 2
    bad("fold 1 holds no negative weight", y_=np.where(fold == 1, 1, y), cv=fold,
        rank_metrics=("auc",))
    w = np.ones(n)
    w[(fold == 0) & (y == 1)] = 0.0
    bad("fold 0 holds no positive weight", cv=fold, sample_weight=w, rank_metrics=("auc",))
    three = np.arange(n) % 3
    y3 = np.where(three == 0, (np.arange(n) // 3) % 2, 0)  # positives in fold 0 only
    bad("fold 1 holds no positive weight", y_=y3, cv=three, rank_metrics=("auc",))
    # valid calls get as far as the fits
    for kw in (dict(rank_metrics=("auc",), select="auc"), dict(rank_metrics="auc"),
               dict(rank_metrics=("auc",), select="auc", metrics=("sign_error",), refit=True)):
        with pytest.raises(AssertionError, match="the device library was asked for"):
            cross_validate_path(clf, X, y, cv=2, gamma=[1.0, 0.1], **kw)


def test_select_picks_the_largest_mean_auc():
    from sparsepoly_amd.model_selection import CVResult

    params = [{"gamma": v} for v in (1.0, 0.1, 0.01)]
    loss = (np.array([3.0, 3, 1, 1, 2, 2]), np.zeros(6))
    auc = (np.array([0.5, 0.7, 0.9, 0.7, 0.7, 0.9]), np.zeros(6))
    r = CVResult(params, np.zeros(4, dtype=np.int32), 2, {"loss": loss, "auc": auc}, None, {})
    assert r.best_index_ == 1                                  # smallest mean loss, as before
    r = CVResult(params, np.zeros(4, dtype=np.int32), 2, {"loss": loss, "auc": auc}, None, {},
                 "loss")
    assert r.best_index_ == 1
    r = CVResult(params, np.zeros(4, dtype=np.int32), 2, {"loss": loss, "auc": auc}, None, {},
                 "auc")
    assert r.best_index_ == 1 and r.best_params_ == params[1]  # 0.8 twice: the lower index
    assert r.mean_test_["auc"].tolist() == [0.6, 0.8, 0.8]
    r = CVResult(params, np.zeros(4, dtype=np.int32), 2, {"auc": auc}, None, {})
    assert r.best_index_ is None


def test_training_auc_is_no_function_of_the_per_fold_tables():
    """Two data sets with the same per-fold AUC, per-fold class counts and per-fold weights, and
    different AUC on the union of folds 1 and 2: whatever ``assemble_cv`` (or anything else) makes
    of per-fold cells is the same for both, so the union needs a set of its own."""
    from sparsepoly_amd.bank import restate_group_auc
    from sparsepoly_amd.model_selection import assemble_cv

    g = np.array([0, 0, 1, 1, 2, 2])
    y = np.array([1.0, -1, 1, -1, 1, -1])
    a = np.array([[2.0, 1, 2, 1, 4, 3]]).T   # fold 2 above fold 1: its negative beats a positive
    b = np.array([[2.0, 1, 4, 1, 3, 2]]).T   # interleaved the other way: every positive on top
    union = np.array([[False, True, True]])
    per_fold, joint = [], []
    for s in (a, b):
        per_fold.append(restate_group_auc(s, y, None, g, 3, None))
        joint.append(restate_group_auc(s, y, None, g, 3, union)["auc"][0, 0])
    assert (per_fold[0]["pairs"] == per_fold[1]["pairs"]).all()
    assert (per_fold[0]["auc"] == 1.0).all()
    assert joint == [0.75, 1.0]
    weight = np.array([2.0, 2.0, 2.0])
    guess = [assemble_cv({"auc": p["auc"] * weight}, weight, [0])["auc"][1][0] for p in per_fold]
    assert guess[0] == guess[1] == 1.0 and guess[0] != joint[0]


def test_header_and_python_agree_on_the_constants():
    import os

    from sparsepoly_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "spfm.h")).read()
    assert "#define SPFM_BANK_MAX_SETS %d\n" % _capi.BANK_MAX_SETS in header
    assert "#define SPFM_BANK_RANK_BLOCK %d\n" % _capi.BANK_RANK_BLOCK in header
    assert "#define SPFM_BANK_AUC_MAX_BYTES (1ll << 30)\n" in header
    assert _capi.BANK_AUC_MAX_BYTES == 1 << 30
    assert "int spfm_bank_group_auc(" in header and "spfm_bank_group_auc" in _capi.SYMBOLS
