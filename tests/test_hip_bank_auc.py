"""``spfm_bank_group_auc``, ``ModelBank.group_auc``, ``cross_validate_path(rank_metrics=)`` and
``roc_auc`` on the device.  Needs a real MI355X: ``pytest -m gpu``.

The yardstick is ``restate_group_auc`` (NumPy; held to an O(n^2) loop and to scikit-learn in
``tests/test_bank_auc_host.py``) applied to the scores of the bank's own ``decision_function``:
what is under test is the key image, the sorts and the walk, not the scoring pass.

Shapes: ``B = SPFM_BANK_RANK_BLOCK`` sorted positions per workgroup of the walk, ``n = 3 B + 37``
rows (four workgroups, the last one short), 12 columns.  Unweighted everything is integers: equal
or wrong.  Weighted, with u = 2^-53, every device quantity is a sum or product of non-negative
doubles (``csrc/spfm_bank_rank.hip.h``): the class weights and the running negatives go through at
most ``B + n / B + 3`` additions, a term is one product and one addition on top, the terms through
as many additions again, numerator over denominator three more roundings: far inside the
``(4 n + 16) u`` relative that holds for any order of those sums (``tests/test_bank_auc_host.py``),
which is the bound asserted here.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
from test_ranking_host import fm

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
D = 12


def _n():
    from sparsepoly_amd import _capi

    return 3 * _capi.BANK_RANK_BLOCK + 37


def _tied_rows(n, seed=3):
    """about 40 distinct rows over the columns 0..10, each repeated, in shuffled order; column 11
    holds a value of its own in every row"""
    rng = np.random.RandomState(seed)
    base = np.where(rng.rand(40, D) < 0.4, rng.randn(40, D), 0.0)
    base[0] = 0.0
    V = base[rng.randint(0, 40, size=n)]
    V[:, D - 1] = rng.permutation(n) + 1.0
    return sp.csr_matrix(V)


def _members():
    """zero: every parameter 0 (one score); tied: blind to column 11 (identical rows give
    bit-identical scores); distinct: a linear weight on column 11 as well"""
    zero, tied, distinct = (fm(2, k, D, None, True, seed=40 + k) for k in (2, 3, 5))
    zero.P_[:] = 0.0
    zero.w_[:] = 0.0
    for e in (tied, distinct):
        e.P_[:, :, D - 1] = 0.0
        e.w_[D - 1] = 0.0
    distinct.w_[D - 1] = 1e-3
    return [zero, tied, distinct]


@pytest.fixture(scope="module")
def case():
    from sparsepoly_amd import ModelBank

    n = _n()
    X = _tied_rows(n)
    ests = _members()
    rng = np.random.RandomState(8)
    y = np.where(rng.rand(n) < 0.3, 1.0, -1.0)
    Y = np.where(rng.rand(n, 3) < 0.5, 1.0, -1.0)
    g = rng.randint(0, 5, size=n).astype(np.int32)
    with ModelBank(ests) as bank:
        scores = bank.decision_function(X)
        # the structure the case is about, from the scores themselves
        B = (n - 37) // 3
        assert len(np.unique(scores[:, 0] + 0.0)) == 1
        runs = np.unique(scores[:, 1], return_counts=True)[1]
        assert len(runs) <= 40 and runs.max() > 10 and n > 3 * B
        assert len(np.unique(scores[:, 2])) == n
        yield bank, ests, X, scores, y, Y, g


def _same(got, want, keys=("auc", "pos_weight", "neg_weight", "pairs")):
    for k in keys:
        assert (k in got) == (k in want), k
        if k in got:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k], want[k], equal_nan=True), k


def _close(got, want, n, what):
    """weighted tables within (4 n + 16) u relative of a wide restatement"""
    tol = (4 * n + 16) * U53
    worst = 0.0
    for k in ("auc", "pos_weight", "neg_weight"):
        a, b = got[k], np.asarray(want[k], dtype=np.double)
        assert a.shape == b.shape and (np.isnan(a) == np.isnan(b)).all(), (what, k)
        ok = ~np.isnan(b)
        err = np.abs(a[ok] - b[ok])
        assert (err <= tol * np.abs(b[ok])).all(), (what, k)
        nz = b[ok] != 0  # (an empty set has weights of exactly 0 on both sides)
        if nz.any():
            worst = max(worst, float((err[nz] / np.abs(b[ok][nz])).max() / tol))
    print("%s: largest error %.3g of its bound" % (what, worst))


# ---------------------------------------------------------------- 1. ties across boundaries
def test_ties_across_block_boundaries_unweighted(case):
    from sparsepoly_amd.bank import restate_group_auc

    bank, ests, X, scores, y, Y, g = case
    got = bank.group_auc(X, y)
    want = restate_group_auc(scores, y, None, None, 1, None)
    assert got["pairs"].shape == (3, 1, 3) and got["pairs"].dtype == np.int64
    assert (got["pairs"] == want["pairs"]).all()
    u2, npos, nneg = (got["pairs"][:, 0, k] for k in range(3))
    assert (npos == (y > 0).sum()).all() and (nneg == (y <= 0).sum()).all()
    assert (got["auc"][:, 0] == u2.astype(np.double) / (2.0 * npos.astype(np.double)
                                                         * nneg.astype(np.double))).all()
    assert got["auc"][0, 0] == 0.5 and u2[0] == npos[0] * nneg[0]  # one run over all rows
    assert (got["pos_weight"][:, 0] == npos).all() and (got["neg_weight"][:, 0] == nneg).all()
    _same(got, want)


# ---------------------------------------------------------------- 2. weighted
def test_integer_weights_equal_replicated_rows(case):
    bank, ests, X, scores, y, Y, g = case
    n = X.shape[0]
    w = np.random.RandomState(2).randint(0, 4, size=n).astype(np.double)
    assert (w == 0).any()
    rep = np.repeat(np.arange(n), w.astype(int))
    sets = np.array([[True] * 5, [True, True, False, False, False], [False] * 4 + [True]])
    got = bank.group_auc(X, y, groups=g, n_groups=5, sample_weight=w, sets=sets)
    flat = bank.group_auc(X[rep], y[rep], groups=g[rep], n_groups=5, sets=sets)
    assert "pairs" not in got
    assert (got["pos_weight"] == flat["pairs"][:, :, 1]).all()
    assert (got["neg_weight"] == flat["pairs"][:, :, 2]).all()
    _close(got, flat, n, "integer weights against replicated rows")


def test_uniform_weights_against_the_wide_restatement(case):
    from sparsepoly_amd.bank import restate_group_auc

    bank, ests, X, scores, y, Y, g = case
    n = X.shape[0]
    w = np.random.RandomState(4).rand(n) + 0.5
    sets = np.array([[True] * 5, [False, True, True, False, True]])
    for t, what in ((y, "shared y"), (Y, "per-member Y")):
        got = bank.group_auc(X, t, groups=g, n_groups=5, sample_weight=w, sets=sets)
        want = restate_group_auc(scores, t, w, g, 5, sets, wide=True)
        _close(got, want, n, "uniform weights, %s" % what)


# ---------------------------------------------------------------- 3. partition, position, repeat
def test_slabs_do_not_change_a_bit(case):
    bank, ests, X, scores, y, Y, g = case
    w = np.random.RandomState(5).rand(X.shape[0]) * 2
    kw = dict(groups=g, n_groups=5)
    one = bank.group_auc(X, Y, **kw), bank.group_auc(X, Y, sample_weight=w, **kw)
    again = bank.group_auc(X, Y, **kw), bank.group_auc(X, Y, sample_weight=w, **kw)
    bank.set_partition(X.nnz // 4)
    try:
        parts = bank.group_auc(X, Y, **kw), bank.group_auc(X, Y, sample_weight=w, **kw)
        assert bank.info()["slabs"] >= 3
    finally:
        bank.set_partition(0)
    for a, b, c in zip(one, again, parts):
        _same(a, b)
        _same(a, c)


def test_batches_of_members_do_not_change_a_bit(case, monkeypatch):
    """the test hook SPFM_BANK_AUC_BATCH caps the members per sort batch: 3 members go as 3 batches of one and as
    batches of two and one, with per-member sets and targets, so every offset by the batch's first
    member (keys, class bytes, set masks, results) and the reuse of the batch buffers is in play"""
    bank, ests, X, scores, y, Y, g = case
    w = np.random.RandomState(6).rand(X.shape[0]) + 0.5
    held = np.array([4, 0, 2])
    own = held[:, None] == np.arange(5)[None, :]
    kw = dict(groups=g, n_groups=5, sets=np.stack([own, ~own, own | ~own], axis=1))
    whole = bank.group_auc(X, Y, **kw), bank.group_auc(X, Y, sample_weight=w, **kw)
    for cap in ("1", "2"):
        monkeypatch.setenv("SPFM_BANK_AUC_BATCH", cap)
        parts = bank.group_auc(X, Y, **kw), bank.group_auc(X, Y, sample_weight=w, **kw)
        for a, b in zip(whole, parts):
            _same(a, b)
    assert len({tuple(p) for p in whole[0]["pairs"][:, 0]}) == 3  # the members differ


def test_a_column_of_a_full_bank_is_the_one_member_bank():
    from sparsepoly_amd import ModelBank

    n = _n()
    X = _tied_rows(n, seed=9)
    ests = [fm(2, 2, D, None, True, seed=700 + f) for f in range(64)]
    for e in ests[::3]:  # members blind to column 11: tie runs
        e.P_[:, :, D - 1] = 0.0
        e.w_[D - 1] = 0.0
    rng = np.random.RandomState(10)
    Y = np.where(rng.rand(n, 64) < 0.5, 1.0, -1.0)
    g = rng.randint(0, 3, size=n).astype(np.int32)
    w = rng.rand(n) + 0.25
    sets = rng.rand(64, 2, 3) < 0.6
    with ModelBank(ests) as b:
        full = b.group_auc(X, Y, groups=g, sets=sets), b.group_auc(X, Y, groups=g, sets=sets,
                                                                    sample_weight=w)
    for f in (0, 31, 63):
        with ModelBank([ests[f]]) as solo:
            col = (solo.group_auc(X, Y[:, f], groups=g, sets=sets[f]),
                   solo.group_auc(X, Y[:, f], groups=g, sets=sets[f], sample_weight=w))
        for a, c in zip(full, col):
            for k in c:
                assert np.array_equal(a[k][f], c[k][0], equal_nan=True), (f, k)


# ---------------------------------------------------------------- 4. sets
def test_held_out_and_complement_per_member(case):
    from sparsepoly_amd.bank import restate_group_auc

    bank, ests, X, scores, y, Y, g = case
    held = np.array([0, 3, 4])
    own = held[:, None] == np.arange(5)[None, :]
    sets = np.stack([own, ~own], axis=1)
    got = bank.group_auc(X, y, groups=g, n_groups=5, sets=sets)
    _same(got, restate_group_auc(scores, y, None, g, 5, sets))
    both = got["pairs"][:, 0, 1:] + got["pairs"][:, 1, 1:]
    assert (both == [(y > 0).sum(), (y <= 0).sum()]).all()
    default = bank.group_auc(X, y, groups=g, n_groups=5)  # sets=None: one set per group
    _same(default, restate_group_auc(scores, y, None, g, 5, None))
    assert (default["pairs"][np.arange(3), held] == got["pairs"][:, 0]).all()


def test_thirty_two_sets_and_a_set_without_a_class(case):
    from sparsepoly_amd.bank import restate_group_auc

    bank, ests, X, scores, y, Y, g = case
    n = X.shape[0]
    rng = np.random.RandomState(12)
    g32 = (rng.permutation(n) % 32).astype(np.int32)
    sets = rng.rand(3, 32, 32) < 0.3
    sets[:, 5] = False                     # an empty set
    sets[:, 6] = False
    sets[:, 6, 31] = True                  # a set of group 31 alone: made negative below
    t = y.copy()
    t[g32 == 31] = -1.0
    w = rng.rand(n) + 0.5
    got = bank.group_auc(X, t, groups=g32, n_groups=32, sets=sets)
    _same(got, restate_group_auc(scores, t, None, g32, 32, sets))
    assert np.isnan(got["auc"][:, 5]).all() and (got["pairs"][:, 5] == 0).all()
    assert np.isnan(got["auc"][:, 6]).all() and (got["pairs"][:, 6, 1] == 0).all()
    assert (got["pairs"][:, 6, 2] == (g32 == 31).sum()).all()
    gw = bank.group_auc(X, t, groups=g32, n_groups=32, sets=sets, sample_weight=w)
    _close(gw, restate_group_auc(scores, t, w, g32, 32, sets, wide=True), n, "U = 32, weighted")
    assert np.isnan(gw["auc"][:, 6]).all() and (gw["neg_weight"][:, 6] > 0).all()


def test_small_shapes():
    from sparsepoly_amd import ModelBank
    from sparsepoly_amd.bank import restate_group_auc

    est = fm(2, 3, D, None, True, seed=77)
    X = _tied_rows(70, seed=1)
    y = np.where(np.arange(70) % 3 == 0, 1.0, -1.0)
    with ModelBank([est]) as b:                                   # F = 1
        s = b.decision_function(X)
        _same(b.group_auc(X, y), restate_group_auc(s, y, None, None, 1, None))
        one = b.group_auc(X[:1], y[:1])                           # n = 1
        assert np.isnan(one["auc"][0, 0]) and one["pairs"][0, 0].tolist() == [0, 1, 0]
        two = b.group_auc(X[:2], np.array([1.0, -1.0]))           # one pair
        u2 = 2 if s[0, 0] > s[1, 0] else 1 if s[0, 0] == s[1, 0] else 0
        assert two["pairs"][0, 0].tolist() == [u2, 1, 1] and two["auc"][0, 0] == u2 / 2.0
    # n = 0: through the C entry (test_entry_point_refusals); the estimators' checks want a row


# ---------------------------------------------------------------- 5. the C entry point's errors
def test_entry_point_refusals(monkeypatch):
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    lib = eng._lib
    d, F, k, n = 6, 2, 3, 3
    lengths = [2, 0, 3]
    rng = np.random.RandomState(1)
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ii = np.array([0, 4, 1, 2, 5], dtype=np.int32)
    dd = rng.randn(5)
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    i32, i64, u32, f64 = C.c_int32, C.c_int64, C.c_uint32, C.c_double
    y = np.array([1.0, -1.0, 1.0])
    out = np.full(64 * 40 * 3, 7.25)
    pairs = np.full(64 * 40 * 3, 7, dtype=np.int64)
    masks = lambda *a: np.array(a, dtype=np.uint32)  # noqa: E731

    def call(n_=n, d_=d, ip_=ip, y_=y, w=None, g=None, G=2, s=None, U=0, o=out, pr=pairs):
        return lib.spfm_bank_group_auc(eng._h, n_, d_, p(ip_, i64), p(ii, i32), p(dd, f64),
                                       p(y_, f64), 0, p(w, f64), p(g, i32), G, p(s, u32), U,
                                       p(o, f64), p(pr, i64))

    def expect(rc, code, text):
        msg = lib.spfm_last_error(eng._h).decode()
        assert rc == code and text in msg, (rc, msg)
        assert (out == 7.25).all() and (pairs == 7).all()  # refused before the first write

    INV, UNS = _capi.SPFM_ERR_INVALID, _capi.SPFM_ERR_UNSUPPORTED
    ids = lambda *a: np.array(a, dtype=np.int32)  # noqa: E731
    try:
        expect(call(), INV, "no bank set")
        eng.bank_set(np.array([0, k, 2 * k]), [2], np.zeros((1, d, 2 * k)), np.ones(2 * k),
                     np.zeros((d, F)))
        # what bank_check refuses for the grouped sums
        expect(call(y_=None), INV, "NULL")
        expect(call(g=ids(0, 2, 1)), INV, "group id 2 of row 1")
        expect(call(g=ids(0, -1, 1)), INV, "group id -1")
        expect(call(w=np.array([1.0, -0.5, 1.0])), INV, "negative or not finite")
        expect(call(w=np.array([1.0, np.nan, 1.0])), INV, "negative or not finite")
        expect(call(G=0), INV, "must be >= 1")
        expect(call(d_=d + 1), INV, "the bank has d = %d" % d)
        expect(call(ip_=ip + 1), INV, "bank_group_auc")
        expect(call(G=_capi.BANK_MAX_GROUPS + 1), UNS,
               "SPFM_BANK_MAX_GROUPS = %d" % _capi.BANK_MAX_GROUPS)
        # its own
        expect(call(s=masks(1, 2, 1, 2), U=0), INV, "U must be >= 1")
        expect(call(s=masks(1, 2, 1, 2), U=-1), INV, "U must be >= 1")
        expect(call(s=np.ones(2 * 33, dtype=np.uint32), U=_capi.BANK_MAX_SETS + 1), UNS,
               "SPFM_BANK_MAX_SETS = %d" % _capi.BANK_MAX_SETS)
        expect(call(s=masks(1, 2, 1, 4), U=2), INV, "set 1 of member 1 names a group at or above")
        assert call(o=None) == INV and (pairs == 7).all()
        # the scratch budget: 64 members on 2^21 empty rows are 9 n F > 2^30 bytes of keys alone
        eng.bank_set(np.arange(65), [2], np.zeros((1, d, 64)), np.ones(64), np.zeros((d, 64)))
        big = 1 << 21
        expect(call(n_=big, ip_=np.zeros(big + 1, dtype=np.int64), y_=np.ones(big)), UNS,
               "bytes, above SPFM_BANK_AUC_MAX_BYTES = %d" % _capi.BANK_AUC_MAX_BYTES)
        # the message's bytes are the header's formula, and the test hook does cap the batch:
        # Fb = min(64, 128 MiB / 12 n) = 5 members, or 1 with SPFM_BANK_AUC_BATCH=1
        import re

        def refused_bytes():
            rc = call(n_=big, ip_=np.zeros(big + 1, dtype=np.int64), y_=np.ones(big))
            assert rc == UNS
            return int(re.search(r"is (\d+) bytes", lib.spfm_last_error(eng._h).decode()).group(1))

        per_member = 12 * big + 40 * (big // _capi.BANK_RANK_BLOCK) * 2  # U = G = 2
        assert refused_bytes() == 9 * big * 64 + 4 * big + 5 * per_member
        monkeypatch.setenv("SPFM_BANK_AUC_BATCH", "1")
        assert refused_bytes() == 9 * big * 64 + 4 * big + 1 * per_member
        monkeypatch.delenv("SPFM_BANK_AUC_BATCH")
        # 100k rows x 64 members x 32 sets, weighted, one batch: keys and classes, rows, weights,
        # sorted pairs, block records (40 bytes per set, member and block) -- a sixth of the budget
        n5, B = 100000, _capi.BANK_RANK_BLOCK
        need = 9 * n5 * 64 + 12 * n5 + 12 * n5 * 64 + 40 * -(-n5 // B) * 32 * 64
        assert 6 * need < _capi.BANK_AUC_MAX_BYTES
        # valid calls: n = 0 gives NaN and zeros, F x U x 3 values and no more
        eng.bank_set(np.array([0, k, 2 * k]), [2], np.zeros((1, d, 2 * k)), np.ones(2 * k),
                     np.zeros((d, F)))
        assert call(n_=0, y_=None, G=3) == 0
        tab = out[:F * 3 * 3].reshape(F, 3, 3)
        assert np.isnan(tab[:, :, 0]).all() and (tab[:, :, 1:] == 0).all()
        assert (out[F * 9:] == 7.25).all()
        assert (pairs[:F * 9] == 0).all() and (pairs[F * 9:] == 7).all()
        # every score is 0 (zero parameters): one positive against one negative, tied
        out[:] = 7.25
        pairs[:] = 7
        assert call(y_=np.array([1.0, -1.0, -1.0]), g=ids(0, 0, 1), s=masks(1, 3, 2, 3), U=2) == 0
        assert pairs[:12].reshape(2, 2, 3).tolist() == [[[1, 1, 1], [2, 1, 2]],
                                                        [[0, 0, 1], [2, 1, 2]]]
        tab = out[:12].reshape(2, 2, 3)
        assert tab[0, 0, 0] == 0.5 and tab[0, 1, 0] == 0.5 and np.isnan(tab[1, 0, 0])
        assert (out[12:] == 7.25).all() and (pairs[12:] == 7).all()
        # weighted: pairs is not written
        pairs[:] = 7
        assert call(w=np.array([2.0, 1.0, 0.0]), y_=np.array([1.0, -1.0, -1.0])) == 0
        assert (pairs == 7).all() and out[:3].tolist() == [0.5, 2.0, 1.0]
        info = eng.bank_info()
        assert len(info) == 4 and info["slabs"] == 1
    finally:
        eng.close()


# ---------------------------------------------------------------- 6. cross-validation, roc_auc
def test_cross_validation_selects_by_auc():
    import warnings

    from sparsepoly_amd import ModelBank, SparseFactorizationMachineClassifier, cross_validate_path
    from sparsepoly_amd.bank import restate_group_auc
    from sparsepoly_amd.synth import make_problem

    n = 300
    X, t = make_problem(n, 40, 5, seed=21)
    X = sp.csr_matrix(X)
    X.data = X.data.astype(np.float32).astype(np.float64)
    # one row in five is positive; the estimator's binarizer makes the later label ("yes") +1
    labels = np.where(np.asarray(t) > np.quantile(t, 0.8), "yes", "no")
    ypm = np.where(labels == "yes", 1.0, -1.0)
    base = SparseFactorizationMachineClassifier(
        solver="pbcd", loss="logistic", regularizer="omegacs", schedule="colored", max_iter=4,
        tol=0, random_state=5, beta=1e-3, gamma=1e-3, alpha=1e-3, n_components=4, precision="f32")
    grid = dict(gamma=[1e-3, 30.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = cross_validate_path(base, X, labels, cv=3, rank_metrics=("auc",), select="auc",
                                  **grid)
        plain = cross_validate_path(base, X, labels, cv=3, **grid)
        clf = base.fit(X, labels)
    K = 3
    assert set(res.test_) == {"loss", "sign_error", "auc"} and res.test_["auc"].shape == (2, K)
    assert res.info_ == dict(banks=1, passes=2, members=[6])
    clones = [e for row in res.estimators_ for e in row]
    held = np.tile(np.arange(K), 2)
    own = held[:, None] == np.arange(K)[None, :]
    with ModelBank(clones) as bank:
        scores = bank.decision_function(X)
    want = restate_group_auc(scores, ypm, None, res.fold_, K, np.stack([own, ~own], axis=1))["auc"]
    assert not np.isnan(want).any()
    assert (res.test_["auc"] == want[:, 0].reshape(2, K)).all()
    assert (res.train_["auc"] == want[:, 1].reshape(2, K)).all()
    np.testing.assert_array_equal(res.mean_test_["auc"], res.test_["auc"].mean(axis=1))
    np.testing.assert_array_equal(res.std_test_["auc"], res.test_["auc"].std(axis=1))
    assert res.best_index_ == int(np.argmax(res.mean_test_["auc"]))
    assert res.best_params_ == res.params[res.best_index_]
    # rank_metrics=(): every field as before, and the other fields do not move with it
    assert set(plain.test_) == {"loss", "sign_error"} and set(plain.mean_test_) == set(plain.test_)
    assert plain.info_ == dict(banks=1, passes=1, members=[6])
    assert plain.best_index_ == int(np.argmin(plain.mean_test_["loss"]))
    assert (plain.fold_ == res.fold_).all() and plain.params == res.params
    for m in plain.test_:
        np.testing.assert_array_equal(plain.test_[m], res.test_[m])
        np.testing.assert_array_equal(plain.train_[m], res.train_[m])
    # roc_auc: the one-set table of the one-member bank, labels through the estimator's own
    with ModelBank([clf]) as solo:
        tab = solo.group_auc(X, ypm)
    assert clf.roc_auc(X, labels) == tab["auc"][0, 0] and 0.5 < tab["auc"][0, 0] <= 1.0
    w = np.random.RandomState(1).rand(n) + 0.5
    with ModelBank([clf]) as solo:
        assert clf.roc_auc(X, labels, sample_weight=w) == solo.group_auc(
            X, ypm, sample_weight=w)["auc"][0, 0]
